// Per-data-set posterior summaries and resampling (include/mdns.h, Part 7).
//
// What the reference's post-processing does per spectrum in a Python loop (musefuse_postprocess.py:112-140,
// checkoutput.py:27-44): lw = w + L over the rows where it is finite, p = exp(lw - max) / sum, then
// `numpy.random.choice(jparent, 4000, p=p)` and the mean / std of every parameter of the draws.  Here the
// moments are the exact weighted ones, quantiles come from the weighted order statistics and the draws are
// numpy's own: Generator(Philox(key=[seed, d])).choice(F, n, p=p).
//
// Layouts (as save_results writes them): w, L [nsamp][ndata], x [nsamp][ndata][ndim], row-major doubles.
//
//   k_post_max / k_post_sums / k_post_var   one wave per (64 consecutive data sets, slice of rows): lane d
//                                           reads row i of its column, so a wave reads 512 contiguous bytes
//                                           of w and L per row.  Slices give the grid enough waves at small
//                                           ndata; their partials go to [slice][ndata][...] and a small
//                                           launch combines them in slice order (no atomics: the same bytes
//                                           every call).  Three passes -- max, then sums with the max known,
//                                           then the centred second moment with the mean known -- so the
//                                           variance keeps its digits when |mean| / std is large.
//   k_post_transpose                        64 rows x 64 data sets through LDS: x into column-contiguous
//                                           doubles [d][k][nsamp], p into fixed-point integer weights
//                                           [d][nsamp] (round(p 2^52); rows outside F weigh 0).
//   k_post_quantile                         one workgroup per (data set, parameter): radix select over the
//                                           order-preserving 64-bit key of x, 8 bits per level, with integer
//                                           weight histograms in LDS.  Integer sums do not depend on the
//                                           order of the adds, so the result is deterministic; the column
//                                           is staged in LDS when it fits and read from the scratch
//                                           otherwise (any nsamp).  The answer is a key that exists: one of
//                                           the sample values.
//   k_post_resample                         one workgroup per data set: a fixed-order scan of exp(lw - max)
//                                           into a cdf over all rows (rows outside F add 0), divided by its
//                                           last element as numpy does; every thread makes whole
//                                           Philox4x64-10 blocks (key = (seed, first column + d), block b at counter b + 1,
//                                           four draws each) and binary-searches with side='right'.
#include "mdns_internal.h"

#include <cmath>
#include <cstdlib>

namespace mdns {

static constexpr int kPostDim = 8;              // parameters per sample at most
static constexpr int kWave = 64;
static constexpr int kQBlock = 256;             // threads of a quantile / resampling workgroup
static constexpr int kQLds = 3840;              // samples a quantile workgroup stages in LDS (60 KiB + the histogram)
static constexpr int kSliceRows = 128;          // rows per slice of the moment passes (at least)
static constexpr int kMaxQ = 64;                // quantiles per call at most
static constexpr double kFix = 4503599627370496.0;   // 2^52: fixed-point scale of the quantile weights
static constexpr size_t kScratchBytes = (size_t) 512 << 20;   // transposed columns / cdfs per batch of data sets

// ---- moments ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kWave) void k_post_max(const double *__restrict__ w, const double *__restrict__ L,
                                                    int nsamp, int ndata, int rows_per_slice,
                                                    double *__restrict__ part_m, int *__restrict__ part_n,
                                                    double *__restrict__ part_L, int *__restrict__ part_arg)
{
	const int d = blockIdx.x * kWave + threadIdx.x;
	if (d >= ndata) return;
	const int lo = blockIdx.y * rows_per_slice;
	const int hi = min(nsamp, lo + rows_per_slice);
	double m = -INFINITY, bestL = -INFINITY;
	int n = 0, arg = -1;
#pragma unroll 4
	for (int i = lo; i < hi; ++i) {
		const size_t at = (size_t) i * ndata + d;
		const double l = L[at];
		const double lw = w[at] + l;
		if (isfinite(lw)) {
			++n;
			m = fmax(m, lw);
			if (arg < 0 || l > bestL) { bestL = l; arg = i; }     // strict: the first row of a tie
		}
	}
	const size_t o = (size_t) blockIdx.y * ndata + d;
	part_m[o] = m; part_n[o] = n; part_L[o] = bestL; part_arg[o] = arg;
}

__global__ __launch_bounds__(256) void k_post_max_combine(const double *__restrict__ part_m, const int *__restrict__ part_n,
                                                          const double *__restrict__ part_L, const int *__restrict__ part_arg,
                                                          int nslices, int ndata, double *__restrict__ m_out,
                                                          int *__restrict__ n_out, int *__restrict__ imax_out)
{
	const int d = blockIdx.x * blockDim.x + threadIdx.x;
	if (d >= ndata) return;
	double m = -INFINITY, bestL = -INFINITY;
	int n = 0, arg = -1;
	for (int s = 0; s < nslices; ++s) {
		const size_t o = (size_t) s * ndata + d;
		n += part_n[o];
		m = fmax(m, part_m[o]);
		if (part_arg[o] >= 0 && (arg < 0 || part_L[o] > bestL)) { bestL = part_L[o]; arg = part_arg[o]; }
	}
	m_out[d] = m; n_out[d] = n; imax_out[d] = arg;
}

// part [slice][ndata][2 + ndim]: sum e, sum e^2, sum e x_k
__global__ __launch_bounds__(kWave) void k_post_sums(const double *__restrict__ w, const double *__restrict__ L,
                                                     const double *__restrict__ x, int nsamp, int ndata, int ndim,
                                                     int rows_per_slice, const double *__restrict__ m_in,
                                                     double *__restrict__ part)
{
	const int d = blockIdx.x * kWave + threadIdx.x;
	if (d >= ndata) return;
	const int lo = blockIdx.y * rows_per_slice;
	const int hi = min(nsamp, lo + rows_per_slice);
	const double m = m_in[d];
	double se = 0.0, se2 = 0.0, sx[kPostDim];
#pragma unroll
	for (int k = 0; k < kPostDim; ++k) sx[k] = 0.0;
	for (int i = lo; i < hi; ++i) {
		const size_t at = (size_t) i * ndata + d;
		const double lw = w[at] + L[at];
		if (!isfinite(lw)) continue;
		const double e = exp(lw - m);
		se += e;
		se2 += e * e;
		const double *xr = x + at * ndim;
#pragma unroll
		for (int k = 0; k < kPostDim; ++k)
			if (k < ndim) sx[k] += e * xr[k];
	}
	double *o = part + ((size_t) blockIdx.y * ndata + d) * (2 + ndim);
	o[0] = se; o[1] = se2;
#pragma unroll
	for (int k = 0; k < kPostDim; ++k)
		if (k < ndim) o[2 + k] = sx[k];
}

__global__ __launch_bounds__(256) void k_post_sums_combine(const double *__restrict__ part, int nslices, int ndata, int ndim,
                                                           const double *__restrict__ m_in, const int *__restrict__ n_in,
                                                           double *__restrict__ S_out, double *__restrict__ log_norm,
                                                           double *__restrict__ ess, double *__restrict__ mean)
{
	const int d = blockIdx.x * blockDim.x + threadIdx.x;
	if (d >= ndata) return;
	const int w = 2 + ndim;
	double se = 0.0, se2 = 0.0, sx[kPostDim];
#pragma unroll
	for (int k = 0; k < kPostDim; ++k) sx[k] = 0.0;
	for (int s = 0; s < nslices; ++s) {
		const double *o = part + ((size_t) s * ndata + d) * w;
		se += o[0]; se2 += o[1];
#pragma unroll
		for (int k = 0; k < kPostDim; ++k)
			if (k < ndim) sx[k] += o[2 + k];
	}
	const bool none = n_in[d] == 0;
	S_out[d] = none ? 0.0 : se;
	log_norm[d] = none ? NAN : m_in[d] + log(se);
	ess[d] = none ? NAN : se * se / se2;
	for (int k = 0; k < ndim; ++k) mean[(size_t) d * ndim + k] = none ? NAN : sx[k] / se;
}

// part [slice][ndata][ndim]: sum e (x_k - mean_k)^2
__global__ __launch_bounds__(kWave) void k_post_var(const double *__restrict__ w, const double *__restrict__ L,
                                                    const double *__restrict__ x, int nsamp, int ndata, int ndim,
                                                    int rows_per_slice, const double *__restrict__ m_in,
                                                    const double *__restrict__ mean, double *__restrict__ part)
{
	const int d = blockIdx.x * kWave + threadIdx.x;
	if (d >= ndata) return;
	const int lo = blockIdx.y * rows_per_slice;
	const int hi = min(nsamp, lo + rows_per_slice);
	const double m = m_in[d];
	double mu[kPostDim], sv[kPostDim];
#pragma unroll
	for (int k = 0; k < kPostDim; ++k) { mu[k] = k < ndim ? mean[(size_t) d * ndim + k] : 0.0; sv[k] = 0.0; }
	for (int i = lo; i < hi; ++i) {
		const size_t at = (size_t) i * ndata + d;
		const double lw = w[at] + L[at];
		if (!isfinite(lw)) continue;
		const double e = exp(lw - m);
		const double *xr = x + at * ndim;
#pragma unroll
		for (int k = 0; k < kPostDim; ++k)
			if (k < ndim) { const double c = xr[k] - mu[k]; sv[k] += e * (c * c); }
	}
	double *o = part + ((size_t) blockIdx.y * ndata + d) * ndim;
#pragma unroll
	for (int k = 0; k < kPostDim; ++k)
		if (k < ndim) o[k] = sv[k];
}

__global__ __launch_bounds__(256) void k_post_var_combine(const double *__restrict__ part, int nslices, int ndata, int ndim,
                                                          const double *__restrict__ S_in, const int *__restrict__ n_in,
                                                          double *__restrict__ std_out)
{
	const int d = blockIdx.x * blockDim.x + threadIdx.x;
	if (d >= ndata) return;
	for (int k = 0; k < ndim; ++k) {
		double v = 0.0;
		for (int s = 0; s < nslices; ++s) v += part[((size_t) s * ndata + d) * ndim + k];
		std_out[(size_t) d * ndim + k] = n_in[d] == 0 ? NAN : sqrt(v / S_in[d]);
	}
}

// ---- quantiles -------------------------------------------------------------------------------------------

// data sets [d0, d0 + dn): xt [dn][ndim][nsamp], wt [dn][nsamp]
__global__ __launch_bounds__(256) void k_post_transpose(const double *__restrict__ w, const double *__restrict__ L,
                                                        const double *__restrict__ x, int nsamp, int ndata, int ndim,
                                                        int d0, int dn, const double *__restrict__ m_in,
                                                        const double *__restrict__ S_in, double *__restrict__ xt,
                                                        unsigned long long *__restrict__ wt)
{
	__shared__ double tile[kWave][kWave + 1];
	const int i0 = blockIdx.x * kWave, dd0 = blockIdx.y * kWave;
	const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
	// weights: lane = data set on the way in, row on the way out
	for (int r = wave; r < kWave; r += 4) {
		const int i = i0 + r, dl = dd0 + lane;
		double v = 0.0;
		if (i < nsamp && dl < dn) {
			const int d = d0 + dl;
			const size_t at = (size_t) i * ndata + d;
			const double lw = w[at] + L[at];
			if (isfinite(lw)) v = rint(exp(lw - m_in[d]) / S_in[d] * kFix);
		}
		tile[r][lane] = v;
	}
	__syncthreads();
	for (int c = wave; c < kWave; c += 4) {
		const int dl = dd0 + c, i = i0 + lane;
		if (dl < dn && i < nsamp) wt[(size_t) dl * nsamp + i] = (unsigned long long) tile[lane][c];
	}
	for (int k = 0; k < ndim; ++k) {
		__syncthreads();
		for (int r = wave; r < kWave; r += 4) {
			const int i = i0 + r, dl = dd0 + lane;
			tile[r][lane] = (i < nsamp && dl < dn) ? x[((size_t) i * ndata + d0 + dl) * ndim + k] : 0.0;
		}
		__syncthreads();
		for (int c = wave; c < kWave; c += 4) {
			const int dl = dd0 + c, i = i0 + lane;
			if (dl < dn && i < nsamp) xt[((size_t) dl * ndim + k) * nsamp + i] = tile[lane][c];
		}
	}
}

// order-preserving key of a double: a < b  <=>  key(a) < key(b) (the two zeros apart)
__device__ __forceinline__ unsigned long long post_key(double v)
{
	const unsigned long long b = (unsigned long long) __double_as_longlong(v);
	return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double post_unkey(unsigned long long k)
{
	return __longlong_as_double((long long) ((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// quant [ndata][ndim][nq] for the data sets of the batch: the smallest value whose cumulative weight reaches
// q * total, found digit by digit from the top of the key
__global__ __launch_bounds__(kQBlock) void k_post_quantile(const double *__restrict__ xt, const unsigned long long *__restrict__ wt,
                                                           int nsamp, int ndim, int d0, const double *__restrict__ q, int nq,
                                                           double *__restrict__ quant)
{
	extern __shared__ unsigned long long post_lds[];          // [nsamp] keys | [nsamp] weights, when the column fits
	__shared__ unsigned long long hist[256];
	__shared__ unsigned long long s_pick[2];                  // chosen digit, weight below it
	const int dl = blockIdx.x / ndim, k = blockIdx.x % ndim;
	const double *col = xt + ((size_t) dl * ndim + k) * nsamp;
	const unsigned long long *wcol = wt + (size_t) dl * nsamp;
	const bool staged = nsamp <= kQLds;
	unsigned long long *keys = post_lds, *wts = post_lds + nsamp;
	if (staged) {
		for (int i = threadIdx.x; i < nsamp; i += kQBlock) { keys[i] = post_key(col[i]); wts[i] = wcol[i]; }
		__syncthreads();
	}
	const int lane = threadIdx.x & (kWave - 1);
	double *out = quant + ((size_t) (d0 + dl) * ndim + k) * nq;
	unsigned long long total = 0;
	for (int j = 0; j < nq; ++j) {
		unsigned long long prefix = 0, below = 0, target = 0;
		for (int level = 0; level < 8; ++level) {
			const int shift = 56 - 8 * level;
			const unsigned long long himask = level == 0 ? 0ull : ~0ull << (shift + 8);
			hist[threadIdx.x] = 0;                        // kQBlock == 256 bins
			__syncthreads();
			for (int i = threadIdx.x; i < nsamp; i += kQBlock) {
				const unsigned long long wi = staged ? wts[i] : wcol[i];
				if (wi == 0) continue;
				const unsigned long long key = staged ? keys[i] : post_key(col[i]);
				if ((key & himask) != prefix) continue;
				atomicAdd(&hist[(key >> shift) & 255], wi);
			}
			__syncthreads();
			if (threadIdx.x < kWave) {
				// lane l owns bins 4l..4l+3; an inclusive scan of the lane sums, then the first bin that reaches
				unsigned long long b4[4], own = 0;
#pragma unroll
				for (int t = 0; t < 4; ++t) { b4[t] = hist[4 * lane + t]; own += b4[t]; }
				unsigned long long inc = own;
#pragma unroll
				for (int off = 1; off < kWave; off <<= 1) {
					const unsigned long long o = __shfl_up(inc, off, kWave);
					if (lane >= off) inc += o;
				}
				if (level == 0 && j == 0) total = __shfl(inc, kWave - 1, kWave);
				if (level == 0) {
					const unsigned long long tot = __shfl(inc, kWave - 1, kWave);
					double t = ceil(q[j] * (double) tot);
					target = t < 1.0 ? 1ull : (t >= (double) tot ? tot : (unsigned long long) t);
				}
				const unsigned long long exc = inc - own;
				const unsigned long long hit = __ballot(below + inc >= target);
				const int first = hit ? __ffsll((long long) hit) - 1 : kWave - 1;
				if (lane == first) {
					unsigned long long c = below + exc;
					int t = 0;
					for (; t < 3; ++t) { if (c + b4[t] >= target) break; c += b4[t]; }
					s_pick[0] = (unsigned long long) (4 * lane + t);
					s_pick[1] = c;
				}
			}
			__syncthreads();
			prefix |= s_pick[0] << shift;
			below = s_pick[1];
			__syncthreads();                              // s_pick and hist are rewritten next level
		}
		if (threadIdx.x == 0) out[j] = total == 0 ? NAN : post_unkey(prefix);
	}
}

// ---- resampling ------------------------------------------------------------------------------------------

__device__ __forceinline__ void philox4x64_10(unsigned long long c[4], unsigned long long k0, unsigned long long k1)
{
#pragma unroll
	for (int r = 0; r < 10; ++r) {
		if (r) { k0 += 0x9E3779B97F4A7C15ull; k1 += 0xBB67AE8584CAA73Bull; }
		const unsigned long long a0 = 0xD2E7470EE14C6C93ull, a1 = 0xCA5A826395121157ull;
		const unsigned long long hi0 = __umul64hi(a0, c[0]), lo0 = a0 * c[0];
		const unsigned long long hi1 = __umul64hi(a1, c[2]), lo1 = a1 * c[2];
		const unsigned long long n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
		c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
	}
}

// data sets [d0, d0 + gridDim.x), one workgroup each; cdf [gridDim.x][nsamp] scratch.  Every thread runs over a
// contiguous run of rows, the runs' sums are added in thread order by one thread, and every row's running sum
// is divided by the grand total -- the last row's own running sum, so that row reads exactly 1, as numpy's
// `cdf /= cdf[-1]`.  index [ndata][n], xdraws [ndata][n][ndim] (or nullptr).
__global__ __launch_bounds__(kQBlock) void k_post_resample(const double *__restrict__ w, const double *__restrict__ L,
                                                           const double *__restrict__ x, int nsamp, int ndata, int ndim,
                                                           int d0, const double *__restrict__ m_in, const int *__restrict__ n_in,
                                                           double *__restrict__ cdf, unsigned long long seed, long long key0,
                                                           int n, int *__restrict__ index, double *__restrict__ xdraws)
{
	__shared__ double run[kQBlock];
	__shared__ double s_total;
	const int dl = blockIdx.x, d = d0 + dl;
	int *idx = index + (size_t) d * n;
	double *xd = xdraws ? xdraws + (size_t) d * n * ndim : nullptr;
	if (n_in[d] == 0) {                                   // the whole workgroup leaves: nothing to draw from
		for (int s = threadIdx.x; s < n; s += kQBlock) {
			idx[s] = -1;
			if (xd) for (int k = 0; k < ndim; ++k) xd[(size_t) s * ndim + k] = NAN;
		}
		return;
	}
	const double m = m_in[d];
	const int chunk = (nsamp + kQBlock - 1) / kQBlock;
	const int lo = min(nsamp, (int) threadIdx.x * chunk), hi = min(nsamp, lo + chunk);
	double *c = cdf + (size_t) dl * nsamp;
	double acc = 0.0;
	for (int i = lo; i < hi; ++i) {
		const size_t at = (size_t) i * ndata + d;
		const double lw = w[at] + L[at];
		acc += isfinite(lw) ? exp(lw - m) : 0.0;
		c[i] = acc;
	}
	run[threadIdx.x] = acc;
	__syncthreads();
	if (threadIdx.x == 0) {
		double s = 0.0;
		for (int t = 0; t < kQBlock; ++t) { const double v = run[t]; run[t] = s; s += v; }
		s_total = s;
	}
	__syncthreads();
	const double prefix = run[threadIdx.x], total = s_total;
	for (int i = lo; i < hi; ++i) c[i] = (prefix + c[i]) / total;
	__syncthreads();                                      // the workgroup's stores, seen by the workgroup (one CU)
	const int nblocks = (n + 3) / 4;
	for (int b = threadIdx.x; b < nblocks; b += kQBlock) {
		unsigned long long r[4] = {(unsigned long long) b + 1ull, 0ull, 0ull, 0ull};
		philox4x64_10(r, seed, (unsigned long long) (key0 + d));
#pragma unroll
		for (int j = 0; j < 4; ++j) {
			const int s = 4 * b + j;
			if (s >= n) break;
			const double u = (double) (r[j] >> 11) * 0x1.0p-53;
			int a = 0, z = nsamp;                         // first row with cdf > u (side='right'); cdf[nsamp-1] = 1 > u
			while (a < z) {
				const int mid = (a + z) >> 1;
				if (c[mid] <= u) a = mid + 1; else z = mid;
			}
			if (a >= nsamp) a = nsamp - 1;
			idx[s] = a;
			if (xd) {
				const double *xr = x + ((size_t) a * ndata + d) * ndim;
				for (int k = 0; k < ndim; ++k) xd[(size_t) s * ndim + k] = xr[k];
			}
		}
	}
}

}  // namespace mdns

using namespace mdns;

// phases timed with events on every call (mdns_posterior_timings)
enum { kTimeMoments, kTimeVar, kTimeQuant, kTimeResample, kTimePhases };

struct mdns_posterior {
	int nsamp = 0, ndata = 0, ndim = 0;
	DeviceBuffer<double> d_w, d_L, d_x;
	int nslices = 1, rows_per_slice = 1;
	// per data set: max of lw, sum of exp(lw - max), rows in F, row of the largest L, and the summaries
	DeviceBuffer<double> d_m, d_S, d_lognorm, d_ess, d_mean, d_std;
	DeviceBuffer<int> d_n, d_imax;
	bool normed = false;
	// slice partials: max pass (m | L of the largest | count | row), sums [S][ndata][2 + ndim]
	DeviceBuffer<double> d_pm, d_pL, d_part;
	DeviceBuffer<int> d_pn, d_parg;
	hipEvent_t ev[kTimePhases + 1] = {};
	double ms[kTimePhases] = {};
};

namespace {

bool post_launch_ok(const char *what)
{
	hipError_t e = hipGetLastError();
	if (e != hipSuccess) { set_error("%s: launch failed: %s", what, hipGetErrorString(e)); return false; }
	return true;
}

// max, count and arg-max of L, then the weighted sums: everything the other passes need (once per handle)
bool post_norm(mdns_posterior *h, hipStream_t st)
{
	if (h->normed) return true;
	const dim3 grid((h->ndata + kWave - 1) / kWave, h->nslices), small((h->ndata + 255) / 256);
	hipLaunchKernelGGL(k_post_max, grid, dim3(kWave), 0, st, h->d_w.get(), h->d_L.get(), h->nsamp, h->ndata, h->rows_per_slice,
	                   h->d_pm.get(), h->d_pn.get(), h->d_pL.get(), h->d_parg.get());
	hipLaunchKernelGGL(k_post_max_combine, small, dim3(256), 0, st, h->d_pm.get(), h->d_pn.get(), h->d_pL.get(), h->d_parg.get(), h->nslices, h->ndata,
	                   h->d_m.get(), h->d_n.get(), h->d_imax.get());
	hipLaunchKernelGGL(k_post_sums, grid, dim3(kWave), 0, st, h->d_w.get(), h->d_L.get(), h->d_x.get(), h->nsamp, h->ndata, h->ndim,
	                   h->rows_per_slice, h->d_m.get(), h->d_part.get());
	hipLaunchKernelGGL(k_post_sums_combine, small, dim3(256), 0, st, h->d_part.get(), h->nslices, h->ndata, h->ndim, h->d_m.get(), h->d_n.get(),
	                   h->d_S.get(), h->d_lognorm.get(), h->d_ess.get(), h->d_mean.get());
	if (!post_launch_ok("mdns_posterior (moments)")) return false;
	h->normed = true;
	return true;
}

bool post_var(mdns_posterior *h, hipStream_t st)
{
	const dim3 grid((h->ndata + kWave - 1) / kWave, h->nslices), small((h->ndata + 255) / 256);
	hipLaunchKernelGGL(k_post_var, grid, dim3(kWave), 0, st, h->d_w.get(), h->d_L.get(), h->d_x.get(), h->nsamp, h->ndata, h->ndim,
	                   h->rows_per_slice, h->d_m.get(), h->d_mean.get(), h->d_part.get());
	hipLaunchKernelGGL(k_post_var_combine, small, dim3(256), 0, st, h->d_part.get(), h->nslices, h->ndata, h->ndim, h->d_S.get(), h->d_n.get(),
	                   h->d_std.get());
	return post_launch_ok("mdns_posterior (std)");
}

// the scratch budget of a call: kScratchBytes, or MDNS_POST_SCRATCH_BYTES where that holds a positive integer
// (tests only: it brings the batch loop within reach of small shapes).  Read at every call, not once per process.
size_t post_scratch_bytes()
{
	const char *s = getenv("MDNS_POST_SCRATCH_BYTES");
	if (!s || !*s) return kScratchBytes;
	char *end = nullptr;
	const long long v = strtoll(s, &end, 10);
	return (end && !*end && v > 0) ? (size_t) v : kScratchBytes;
}

// data sets per batch whose scratch (per data set: `per` bytes) fits in the budget
int post_batch(const mdns_posterior *h, size_t per)
{
	size_t b = post_scratch_bytes() / (per ? per : 1);
	if (b < 1) b = 1;
	return b >= (size_t) h->ndata ? h->ndata : (int) b;
}

bool post_elapsed(mdns_posterior *h, int first, int last)
{
	for (int p = first; p < last; ++p) {
		float t = 0.f;
		if (!MDNS_HIP(hipEventElapsedTime(&t, h->ev[p], h->ev[p + 1]))) return false;
		h->ms[p] = t;
	}
	return true;
}

template <class T> bool post_fetch(T *host, const T *dev, size_t count, hipStream_t st)
{
	return !host || MDNS_HIP(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, st));
}

}  // namespace

extern "C" void mdns_posterior_destroy(mdns_posterior *h)
{
	if (!h) return;
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	for (hipEvent_t e : h->ev) if (e) (void) hipEventDestroy(e);
	delete h;
}

extern "C" mdns_posterior *mdns_posterior_create(const double *w, const double *L, const double *x, int nsamp, int ndata, int ndim)
{
	Context *c = ctx();
	if (!c) return nullptr;
	if (!w || !L || !x || nsamp <= 0 || ndata <= 0 || ndim <= 0 || ndim > kPostDim) {
		set_error("mdns_posterior_create: bad arguments (nsamp=%d ndata=%d ndim=%d; 1 <= ndim <= %d)", nsamp, ndata, ndim, kPostDim);
		return nullptr;
	}
	mdns_posterior *h = new mdns_posterior();
	h->nsamp = nsamp; h->ndata = ndata; h->ndim = ndim;
	// slices of 128 rows (fewer than 64 slices: longer ones): 13 at nsamp = 1651, which gives the ~157 column
	// groups of 10 000 data sets 8 waves per CU.  The cut depends on nsamp alone, so a data set sums its rows in
	// the same order whatever the other columns are: the summary of a .cols part equals that of the whole file.
	const int rows = (nsamp + 63) / 64;
	h->rows_per_slice = rows > kSliceRows ? rows : kSliceRows;
	h->nslices = (nsamp + h->rows_per_slice - 1) / h->rows_per_slice;
	const size_t nd = (size_t) ndata, ns = (size_t) nsamp, ps = (size_t) h->nslices * nd;
	bool ok = true;
	for (hipEvent_t &e : h->ev) ok = ok && MDNS_HIP(hipEventCreate(&e));
	ok = ok &&
	    h->d_w.make(ns * nd) && h->d_L.make(ns * nd) && h->d_x.make(ns * nd * ndim) &&
	    h->d_m.make(nd) && h->d_S.make(nd) && h->d_lognorm.make(nd) && h->d_ess.make(nd) &&
	    h->d_mean.make(nd * ndim) && h->d_std.make(nd * ndim) && h->d_n.make(nd) && h->d_imax.make(nd) &&
	    h->d_pm.make(ps) && h->d_pL.make(ps) && h->d_pn.make(ps) && h->d_parg.make(ps) &&
	    h->d_part.make(ps * (2 + ndim)) &&
	    MDNS_HIP(hipMemcpyAsync(h->d_w.get(), w, ns * nd * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipMemcpyAsync(h->d_L.get(), L, ns * nd * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipMemcpyAsync(h->d_x.get(), x, ns * nd * ndim * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipStreamSynchronize(c->stream));
	if (!ok) { mdns_posterior_destroy(h); return nullptr; }      // (it also destroys the events)
	return h;
}

extern "C" int mdns_posterior_summary(mdns_posterior *h, const double *q, int nq, int *nfinite, double *log_norm, double *ess,
                                      double *mean, double *std, double *quant, int *imaxL)
{
	Context *c = ctx();
	if (!c || !h) { if (c) set_error("mdns_posterior_summary: null handle"); return 1; }
	if (quant && (nq <= 0 || nq > kMaxQ || !q)) { set_error("mdns_posterior_summary: nq=%d (1..%d quantiles)", nq, kMaxQ); return 1; }
	if (quant) for (int j = 0; j < nq; ++j)
		if (!(q[j] > 0.0 && q[j] <= 1.0)) { set_error("mdns_posterior_summary: q[%d]=%g outside (0, 1]", j, q[j]); return 1; }
	hipStream_t st = c->stream;
	const size_t nd = (size_t) h->ndata, ndim = (size_t) h->ndim;
	DeviceBuffer<double> q_buf, quant_buf, xt_buf;              // of this call (free themselves)
	DeviceBuffer<unsigned long long> wt_buf;
	const int dbatch = post_batch(h, (size_t) h->nsamp * (ndim + 1) * sizeof(double));
	bool ok = !quant ||
	          (q_buf.make(nq) && quant_buf.make(nd * ndim * nq) && xt_buf.make((size_t) dbatch * ndim * h->nsamp) &&
	           wt_buf.make((size_t) dbatch * h->nsamp) &&
	           MDNS_HIP(hipMemcpyAsync(q_buf.get(), q, nq * sizeof(double), hipMemcpyHostToDevice, st)));
	double *const d_q = q_buf.get(), *const d_quant = quant_buf.get(), *const d_xt = xt_buf.get();
	unsigned long long *const d_wt = wt_buf.get();
	ok = ok && MDNS_HIP(hipEventRecord(h->ev[kTimeMoments], st)) && post_norm(h, st) &&
	     MDNS_HIP(hipEventRecord(h->ev[kTimeVar], st)) && (!std || post_var(h, st)) &&
	     MDNS_HIP(hipEventRecord(h->ev[kTimeQuant], st));
	if (ok && quant) {
		const size_t lds = h->nsamp <= kQLds ? (size_t) 2 * h->nsamp * sizeof(unsigned long long) : 0;
		for (int d0 = 0; ok && d0 < h->ndata; d0 += dbatch) {
			const int dn = h->ndata - d0 < dbatch ? h->ndata - d0 : dbatch;
			hipLaunchKernelGGL(k_post_transpose, dim3((h->nsamp + kWave - 1) / kWave, (dn + kWave - 1) / kWave), dim3(256), 0, st,
			                   h->d_w.get(), h->d_L.get(), h->d_x.get(), h->nsamp, h->ndata, h->ndim, d0, dn, h->d_m.get(), h->d_S.get(), d_xt, d_wt);
			hipLaunchKernelGGL(k_post_quantile, dim3(dn * h->ndim), dim3(kQBlock), lds, st, d_xt, d_wt, h->nsamp, h->ndim, d0,
			                   d_q, nq, d_quant);
			ok = post_launch_ok("mdns_posterior_summary (quantiles)");
		}
	}
	ok = ok && MDNS_HIP(hipEventRecord(h->ev[kTimeResample], st)) &&
	     post_fetch(nfinite, h->d_n.get(), nd, st) && post_fetch(imaxL, h->d_imax.get(), nd, st) &&
	     post_fetch(log_norm, h->d_lognorm.get(), nd, st) && post_fetch(ess, h->d_ess.get(), nd, st) &&
	     post_fetch(mean, h->d_mean.get(), nd * ndim, st) && post_fetch(std, h->d_std.get(), nd * ndim, st) &&
	     (!quant || post_fetch(quant, (const double *) d_quant, nd * ndim * nq, st)) &&
	     MDNS_HIP(hipStreamSynchronize(st)) && post_elapsed(h, kTimeMoments, kTimeResample);
	if (!ok) (void) hipStreamSynchronize(st);                  // (before the call's blocks go)
	return ok ? 0 : 1;
}

extern "C" int mdns_posterior_resample(mdns_posterior *h, unsigned long long seed, long long first_column, int n, int *index,
                                       double *xdraws)
{
	Context *c = ctx();
	if (!c || !h) { if (c) set_error("mdns_posterior_resample: null handle"); return 1; }
	if (n <= 0 || !index) { set_error("mdns_posterior_resample: n=%d, index %s", n, index ? "given" : "NULL"); return 1; }
	hipStream_t st = c->stream;
	const size_t nd = (size_t) h->ndata, ndim = (size_t) h->ndim;
	DeviceBuffer<int> index_buf;                                // of this call (free themselves)
	DeviceBuffer<double> xd_buf, cdf_buf;
	const int dbatch = post_batch(h, (size_t) h->nsamp * sizeof(double));
	bool ok = index_buf.make(nd * n) && (!xdraws || xd_buf.make(nd * n * ndim)) && cdf_buf.make((size_t) dbatch * h->nsamp) &&
	          post_norm(h, st) && MDNS_HIP(hipEventRecord(h->ev[kTimeResample], st));
	int *const d_index = index_buf.get();
	double *const d_xd = xd_buf.get(), *const d_cdf = cdf_buf.get();
	for (int d0 = 0; ok && d0 < h->ndata; d0 += dbatch) {
		const int dn = h->ndata - d0 < dbatch ? h->ndata - d0 : dbatch;
		hipLaunchKernelGGL(k_post_resample, dim3(dn), dim3(kQBlock), 0, st, h->d_w.get(), h->d_L.get(), h->d_x.get(), h->nsamp, h->ndata, h->ndim,
		                   d0, h->d_m.get(), h->d_n.get(), d_cdf, seed, first_column, n, d_index, d_xd);
		ok = post_launch_ok("mdns_posterior_resample");
	}
	ok = ok && MDNS_HIP(hipEventRecord(h->ev[kTimePhases], st)) &&
	     post_fetch(index, (const int *) d_index, nd * n, st) && post_fetch(xdraws, (const double *) d_xd, nd * n * ndim, st) &&
	     MDNS_HIP(hipStreamSynchronize(st));
	if (ok) {
		float t = 0.f;
		ok = MDNS_HIP(hipEventElapsedTime(&t, h->ev[kTimeResample], h->ev[kTimePhases]));
		h->ms[kTimeResample] = t;
	}
	if (!ok) (void) hipStreamSynchronize(st);                  // (before the call's blocks go)
	return ok ? 0 : 1;
}

extern "C" int mdns_posterior_timings(const mdns_posterior *h, double *ms)
{
	if (!h || !ms) { set_error("mdns_posterior_timings: null argument"); return 1; }
	for (int p = 0; p < kTimePhases; ++p) ms[p] = h->ms[p];
	return 0;
}
