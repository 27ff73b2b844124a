// The scale-marginalised likelihood (K2, cmuselike.c:45-64) with a polynomial continuum profiled out PER SPECTRUM
// (include/mdns.h Part 8).  With w = 1/v, the basis b_k(x_j) = Legendre P_k(t_j), k < P <= 4,
// t_j = (2 x_j - x_0 - x_last) / (x_last - x_0):
//
//   once per spectrum      G = sum_j w b b^T,  beta = G^-1 sum_j w b y,  yt = y - sum_k beta_k b_k
//   per (template m, spectrum)
//                          alpha = G^-1 sum_j w b m,  mt = m - sum_k alpha_k b_k,
//                          s = sum w yt mt / (1e-10 + sum w mt^2),  L = -0.5 sum w (yt - s mt)^2
//
// the weighted least-squares minimum over (s, c_0..c_{P-1}) of sum w (y - s m - sum c_k b_k)^2 with the reference's
// 1e-10 on the part of the template the basis cannot express; the fitted continuum is c = beta - s alpha.  Computed in
// this order -- residualise, sum, form the residual -- and not as q0 - a^2/c: at S/N 1000 sum w y^2 is 1e4 times chi^2.
//
// k_continuum_setup        per spectrum G's Cholesky factor and beta (one workgroup per spectrum, sums in a fixed order);
//                          a pivot that is not positive against its diagonal entry raises a status word.
// k_continuum_rows<NP, P>  the role of k_muse_rows: a workgroup keeps yt, w and t of a spectrum in registers (NP channel
//                          pairs per thread), and per template makes three block reductions: sum w b_k m (P sums);
//                          sum w yt mt and sum w mt^2 after alpha's two triangular solves (every thread, redundantly);
//                          sum w r^2.  Basis values come from t by the Legendre recurrence each time.
// k_continuum_rows_generic nx > 4096: the same three reductions as passes over the row from memory.
//
// ONE VALUE PER PAIR: a workgroup scores one candidate at a time, a thread sums its channels in ascending order, a wave
// by wave_sum, the workgroup as (w0 + w1) + (w2 + w3).  The instantiation follows from nx and P alone.  So the bits of
// L for a (template, spectrum) pair do not depend on B, M, the pair's place in the batch, the grid split over the
// candidates or the entry point.
#include "mdns_internal.h"
#include <climits>

namespace mdns {

static constexpr int kBlock = 256;

// Legendre P_0..P_{P-1} at t by the recurrence k P_k = (2k - 1) t P_{k-1} - (k - 1) P_{k-2}
template <int P>
__device__ __forceinline__ void legendre(double t, double (&b)[P])
{
	b[0] = 1.0;
	if constexpr (P > 1) b[1] = t;
	if constexpr (P > 2) b[2] = fma(1.5 * t, b[1], -0.5);
	if constexpr (P > 3) b[3] = fma((5.0 / 3.0) * t, b[2], -(2.0 / 3.0) * b[1]);
}

// v - sum_k c_k b_k, k ascending
template <int P>
__device__ __forceinline__ double residual(double v, const double (&c)[P], const double (&b)[P])
{
#pragma unroll
	for (int k = 0; k < P; k++) v = fma(-c[k], b[k], v);
	return v;
}

// a spectrum's record of d_cfac: off-diagonal entries (k, i), i < k, at k (k - 1) / 2 + i; reciprocal diagonal at 6 + k;
// beta at 10 + k
template <int P>
struct ContFactor {
	double l[6], inv[P], beta[P];
	__device__ __forceinline__ void load(const double *__restrict__ rec)
	{
#pragma unroll
		for (int i = 0; i < P * (P - 1) / 2; i++) l[i] = rec[i];
#pragma unroll
		for (int k = 0; k < P; k++) { inv[k] = rec[6 + k]; beta[k] = rec[10 + k]; }
	}
	// G^-1 c through the two triangular solves, in place
	__device__ __forceinline__ void solve(double (&c)[P]) const
	{
#pragma unroll
		for (int k = 0; k < P; k++) {
			double v = c[k];
#pragma unroll
			for (int i = 0; i < k; i++) v = fma(-l[k * (k - 1) / 2 + i], c[i], v);
			c[k] = v * inv[k];
		}
#pragma unroll
		for (int k = P - 1; k >= 0; k--) {
			double v = c[k];
#pragma unroll
			for (int i = k + 1; i < P; i++) v = fma(-l[i * (i - 1) / 2 + k], c[i], v);
			c[k] = v * inv[k];
		}
	}
};

// N sums over the 256 threads with one barrier, every value by itself: wave_sum, then (w0 + w1) + (w2 + w3).  `slot`
// [4][N] must not be in use by a reduction that other waves may still be reading.
template <int N>
__device__ __forceinline__ void block_sums_each(double (&v)[N], double *slot)
{
	const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
	for (int i = 0; i < N; i++) {
		const double t = wave_sum(v[i]);
		if (lane == 0) slot[wv * N + i] = t;
	}
	__syncthreads();
#pragma unroll
	for (int i = 0; i < N; i++) v[i] = (slot[i] + slot[N + i]) + (slot[2 * N + i] + slot[3 * N + i]);
}

// t [ldm]: the channels mapped to [-1, 1], zero behind channel nx (one channel: t = 0)
__global__ __launch_bounds__(kBlock) void k_continuum_t(const double *__restrict__ x, int nx, double *__restrict__ t, int ldm)
{
	const int j = blockIdx.x * kBlock + threadIdx.x;
	if (j >= ldm) return;
	const double x0 = x[0], x1 = x[nx - 1];
	t[j] = j < nx && x1 != x0 ? (2.0 * x[j] - x0 - x1) / (x1 - x0) : 0.0;
}

// per spectrum: G = sum w b b^T and sum w b y (a thread its channels tid, tid + 256, ... ascending, then
// block_sums_each), the Cholesky factor and beta by thread 0.  A pivot that is not above 1e-13 of its diagonal entry
// (NaN included): fewer than P channels carry weight; *status takes the lowest such spectrum and its record is zeros.
template <int P>
__global__ __launch_bounds__(kBlock) void k_continuum_setup(
    const double *__restrict__ Y, const double *__restrict__ W, int ld, int nx, const double *__restrict__ T, int ndata,
    double *__restrict__ fac, int *__restrict__ status)
{
	constexpr int NG = P * (P + 1) / 2, N = NG + P;
	__shared__ double red[4 * N];
	for (int row = blockIdx.x; row < ndata; row += gridDim.x) {
		const double *yr = Y + (size_t) row * ld, *wr = W + (size_t) row * ld;
		double sums[N];
#pragma unroll
		for (int i = 0; i < N; i++) sums[i] = 0.0;
		for (int j = threadIdx.x; j < nx; j += kBlock) {
			double b[P];
			legendre<P>(T[j], b);
			const double w = wr[j], y = yr[j];
#pragma unroll
			for (int k = 0; k < P; k++) {
				const double wb = w * b[k];
#pragma unroll
				for (int i = 0; i <= k; i++) sums[k * (k + 1) / 2 + i] = fma(wb, b[i], sums[k * (k + 1) / 2 + i]);
				sums[NG + k] = fma(wb, y, sums[NG + k]);
			}
		}
		block_sums_each<N>(sums, red);
		__syncthreads();                                   // (red is written again for the next spectrum)
		if (threadIdx.x != 0) continue;
		double L[P][P], inv[P];
		bool bad = false;
#pragma unroll
		for (int k = 0; k < P; k++) {
#pragma unroll
			for (int i = 0; i <= k; i++) {
				double v = sums[k * (k + 1) / 2 + i];
#pragma unroll
				for (int q = 0; q < i; q++) v = fma(-L[k][q], L[i][q], v);
				if (i == k) {
					if (!(v > 1e-13 * sums[k * (k + 1) / 2 + k]) || !(v < INFINITY)) { bad = true; v = 1.0; }
					L[k][k] = sqrt(v);
					inv[k] = 1.0 / L[k][k];
				} else L[k][i] = v * inv[i];
			}
		}
		double *rec = fac + (size_t) row * kContRec;
		if (bad) {
			atomicMin(status, row);
			for (int i = 0; i < kContRec; i++) rec[i] = 0.0;
			continue;
		}
		ContFactor<P> f;
#pragma unroll
		for (int k = 0; k < P; k++) {
#pragma unroll
			for (int i = 0; i < k; i++) f.l[k * (k - 1) / 2 + i] = L[k][i];
			f.inv[k] = inv[k];
		}
		double beta[P];
#pragma unroll
		for (int k = 0; k < P; k++) beta[k] = sums[NG + k];
		f.solve(beta);
		for (int i = 0; i < kContRec; i++) rec[i] = 0.0;
#pragma unroll
		for (int i = 0; i < P * (P - 1) / 2; i++) rec[i] = f.l[i];
#pragma unroll
		for (int k = 0; k < P; k++) { rec[6 + k] = inv[k]; rec[10 + k] = beta[k]; }
	}
}

// what thread 0 leaves of a scored pair
template <int P>
__device__ __forceinline__ void continuum_store(size_t at, double chi, double s, const ContFactor<P> &f, const double (&alpha)[P],
                                                double *__restrict__ out, double *__restrict__ scale_out, double *__restrict__ coef_out)
{
	out[at] = -0.5 * chi;
	if (scale_out) scale_out[at] = s;
	if (coef_out) {
#pragma unroll
		for (int k = 0; k < P; k++) coef_out[at * P + k] = fma(-s, alpha[k], f.beta[k]);
	}
}

// NP = channel pairs per thread (nx <= 512 NP); templates [B][ldm], zero behind channel nx.  Threads past the last
// channel hold w = 0 and contribute +0 to every sum.  grid.y splits the candidates in chunks of `bchunk`.
template <int NP, int P>
__global__ __launch_bounds__(kBlock) void k_continuum_rows(
    const double *__restrict__ Y, const double *__restrict__ W, int ld, int nx, const double *__restrict__ T,
    const double *__restrict__ fac, const double *__restrict__ model, int ldm, int B, const int *__restrict__ rows, int M,
    double *__restrict__ out, int bchunk, double *__restrict__ scale_out, double *__restrict__ coef_out)
{
	const int bbeg = blockIdx.y * bchunk;
	const int bend = min(B, bbeg + bchunk);
	__shared__ double redA[4 * P], redB[4 * 2], redC[4];
	const int ch = 2 * threadIdx.x;
	bool valid[NP];
	double2 t[NP];
#pragma unroll
	for (int p = 0; p < NP; p++) {
		valid[p] = (p * 512 + ch) < nx;
		t[p] = valid[p] ? *reinterpret_cast<const double2 *>(T + p * 512 + ch) : make_double2(0.0, 0.0);
	}
	for (int k = blockIdx.x; k < M; k += gridDim.x) {
		const int row = rows ? rows[k] : k;
		const size_t base = (size_t) row * ld + ch;
		ContFactor<P> f;
		f.load(fac + (size_t) row * kContRec);
		double2 yt[NP], w[NP];
#pragma unroll
		for (int p = 0; p < NP; p++) {
			// (for odd nx the pad channel of the last pair has y = w = 0: the buffers are zero-filled before the upload)
			const double2 y = valid[p] ? *reinterpret_cast<const double2 *>(Y + base + p * 512) : make_double2(0.0, 0.0);
			w[p] = valid[p] ? *reinterpret_cast<const double2 *>(W + base + p * 512) : make_double2(0.0, 0.0);
			double b0[P], b1[P];
			legendre<P>(t[p].x, b0);
			legendre<P>(t[p].y, b1);
			yt[p] = make_double2(residual<P>(y.x, f.beta, b0), residual<P>(y.y, f.beta, b1));
		}
		for (int b = bbeg; b < bend; b++) {
			const double *mrow = model + (size_t) b * ldm + ch;
			double2 m[NP];
			double alpha[P];
#pragma unroll
			for (int i = 0; i < P; i++) alpha[i] = 0.0;
#pragma unroll
			for (int p = 0; p < NP; p++) {
				m[p] = valid[p] ? *reinterpret_cast<const double2 *>(mrow + p * 512) : make_double2(0.0, 0.0);
				double b0[P], b1[P];
				legendre<P>(t[p].x, b0);
				legendre<P>(t[p].y, b1);
				const double wm0 = w[p].x * m[p].x, wm1 = w[p].y * m[p].y;
#pragma unroll
				for (int i = 0; i < P; i++) { alpha[i] = fma(wm0, b0[i], alpha[i]); alpha[i] = fma(wm1, b1[i], alpha[i]); }
			}
			block_sums_each<P>(alpha, redA);
			f.solve(alpha);
			double ac[2] = {0.0, 0.0};
#pragma unroll
			for (int p = 0; p < NP; p++) {
				double b0[P], b1[P];
				legendre<P>(t[p].x, b0);
				legendre<P>(t[p].y, b1);
				m[p] = make_double2(residual<P>(m[p].x, alpha, b0), residual<P>(m[p].y, alpha, b1));
				const double wm0 = w[p].x * m[p].x, wm1 = w[p].y * m[p].y;
				ac[0] = fma(wm0, yt[p].x, ac[0]);
				ac[0] = fma(wm1, yt[p].y, ac[0]);
				ac[1] = fma(wm0, m[p].x, ac[1]);
				ac[1] = fma(wm1, m[p].y, ac[1]);
			}
			block_sums_each<2>(ac, redB);
			const double s = ac[0] / (1e-10 + ac[1]);             // cmuselike.c:52,57 on the residualised pair
			double chi[1] = {0.0};
#pragma unroll
			for (int p = 0; p < NP; p++) {
				const double r0 = fma(-s, m[p].x, yt[p].x);
				const double r1 = fma(-s, m[p].y, yt[p].y);
				chi[0] = fma(r0 * r0, w[p].x, chi[0]);
				chi[0] = fma(r1 * r1, w[p].y, chi[0]);
			}
			// (redA is written again only by a wave that passed this barrier: everybody has read it by then)
			block_sums_each<1>(chi, redC);
			if (threadIdx.x == 0) continuum_store<P>((size_t) b * M + k, chi[0], s, f, alpha, out, scale_out, coef_out);
		}
	}
}

// any nx: the three reductions as passes over the row from memory
template <int P>
__global__ __launch_bounds__(kBlock) void k_continuum_rows_generic(
    const double *__restrict__ Y, const double *__restrict__ W, int ld, int nx, const double *__restrict__ T,
    const double *__restrict__ fac, const double *__restrict__ model, int ldm, int B, const int *__restrict__ rows, int M,
    double *__restrict__ out, int bchunk, double *__restrict__ scale_out, double *__restrict__ coef_out)
{
	const int bbeg = blockIdx.y * bchunk;
	const int bend = min(B, bbeg + bchunk);
	__shared__ double redA[4 * P], redB[4 * 2], redC[4];
	for (int k = blockIdx.x; k < M; k += gridDim.x) {
		const int row = rows ? rows[k] : k;
		const double *yr = Y + (size_t) row * ld, *wr = W + (size_t) row * ld;
		ContFactor<P> f;
		f.load(fac + (size_t) row * kContRec);
		for (int b = bbeg; b < bend; b++) {
			const double *mr = model + (size_t) b * ldm;
			double alpha[P];
#pragma unroll
			for (int i = 0; i < P; i++) alpha[i] = 0.0;
			for (int j = threadIdx.x; j < nx; j += kBlock) {
				double bv[P];
				legendre<P>(T[j], bv);
				const double wm = wr[j] * mr[j];
#pragma unroll
				for (int i = 0; i < P; i++) alpha[i] = fma(wm, bv[i], alpha[i]);
			}
			block_sums_each<P>(alpha, redA);
			f.solve(alpha);
			double ac[2] = {0.0, 0.0};
			for (int j = threadIdx.x; j < nx; j += kBlock) {
				double bv[P];
				legendre<P>(T[j], bv);
				const double ytj = residual<P>(yr[j], f.beta, bv), mtj = residual<P>(mr[j], alpha, bv);
				const double wm = wr[j] * mtj;
				ac[0] = fma(wm, ytj, ac[0]);
				ac[1] = fma(wm, mtj, ac[1]);
			}
			block_sums_each<2>(ac, redB);
			const double s = ac[0] / (1e-10 + ac[1]);
			double chi[1] = {0.0};
			for (int j = threadIdx.x; j < nx; j += kBlock) {
				double bv[P];
				legendre<P>(T[j], bv);
				const double ytj = residual<P>(yr[j], f.beta, bv), mtj = residual<P>(mr[j], alpha, bv);
				const double r = fma(-s, mtj, ytj);
				chi[0] = fma(r * r, wr[j], chi[0]);
			}
			block_sums_each<1>(chi, redC);
			if (threadIdx.x == 0) continuum_store<P>((size_t) b * M + k, chi[0], s, f, alpha, out, scale_out, coef_out);
		}
	}
}

template <int P>
static void continuum_launch(const mdns_spectra *s, const double *d_model, int ldm, int B, const int *d_rows, int M, double *d_out,
                             double *d_scale, double *d_coef, dim3 grid, int bchunk, hipStream_t stream)
{
	const int nx = s->nx;
#define CONT_ARGS (const double *) s->d_y.get(), (const double *) s->d_w.get(), s->ld, nx, (const double *) s->d_ct.get(), (const double *) s->d_cfac.get(), \
		d_model, ldm, B, d_rows, M, d_out, bchunk, d_scale, d_coef
	if (nx <= 512) hipLaunchKernelGGL((k_continuum_rows<1, P>), grid, dim3(kBlock), 0, stream, CONT_ARGS);
	else if (nx <= 1024) hipLaunchKernelGGL((k_continuum_rows<2, P>), grid, dim3(kBlock), 0, stream, CONT_ARGS);
	else if (nx <= 2048) hipLaunchKernelGGL((k_continuum_rows<4, P>), grid, dim3(kBlock), 0, stream, CONT_ARGS);
	else if (nx <= 4096) hipLaunchKernelGGL((k_continuum_rows<8, P>), grid, dim3(kBlock), 0, stream, CONT_ARGS);
	else hipLaunchKernelGGL((k_continuum_rows_generic<P>), grid, dim3(kBlock), 0, stream, CONT_ARGS);
#undef CONT_ARGS
}

bool launch_continuum_rows(const mdns_spectra *s, const double *d_model, int ldm, int B, const int *d_rows, int M,
                           double *d_out, double *d_scale, double *d_coef)
{
	Context *c = ctx();
	const int P = s->continuum;
	if (P < 1 || P > kContMax || !s->d_ct.get() || !s->d_cfac.get()) { set_error("launch_continuum_rows: no continuum is set on these spectra"); return false; }
	if (B <= 0 || M <= 0) return true;
	int blocks = M < c->num_cus * 8 ? M : c->num_cus * 8;
	// few rows, several candidates: split the candidates over grid.y until ~2 workgroups per CU (as launch_muse_rows)
	int gy = 2 * blocks <= c->num_cus ? (2 * c->num_cus + blocks - 1) / blocks : 1;
	if (gy > B) gy = B;
	const int bchunk = (B + gy - 1) / gy;
	gy = (B + bchunk - 1) / bchunk;
	ProfileScope prof(1);
	const int nx = s->nx;
	if (nx <= 4096) note_kernel(1, "k_continuum_rows<%d, %d>", nx <= 512 ? 1 : nx <= 1024 ? 2 : nx <= 2048 ? 4 : 8, P);
	else note_kernel(1, "k_continuum_rows_generic<%d>", P);
	const dim3 grid(blocks, gy);
	switch (P) {
	case 1: continuum_launch<1>(s, d_model, ldm, B, d_rows, M, d_out, d_scale, d_coef, grid, bchunk, c->stream); break;
	case 2: continuum_launch<2>(s, d_model, ldm, B, d_rows, M, d_out, d_scale, d_coef, grid, bchunk, c->stream); break;
	case 3: continuum_launch<3>(s, d_model, ldm, B, d_rows, M, d_out, d_scale, d_coef, grid, bchunk, c->stream); break;
	default: continuum_launch<4>(s, d_model, ldm, B, d_rows, M, d_out, d_scale, d_coef, grid, bchunk, c->stream); break;
	}
	return launched("k_continuum_rows");
}

}  // namespace mdns

using namespace mdns;

extern "C" int mdns_spectra_continuum(const mdns_spectra *s) { return s ? s->continuum : -1; }

extern "C" int mdns_spectra_set_continuum(mdns_spectra *s, int P)
{
	Context *c = ctx();
	if (!c) return 1;
	if (!s) { set_error("mdns_spectra_set_continuum: null spectra handle"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_continuum: a joint state exists on these spectra (set the continuum first)"); return 1; }
	if (P < 0 || P > kContMax) { set_error("mdns_spectra_set_continuum: P=%d (0: off, 1..%d terms)", P, kContMax); return 1; }
	if (P == 0) {
		if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
		s->d_ct.release(); s->d_cfac.release();
		s->continuum = 0;
		return 0;
	}
	if (!s->d_w.get() || !s->d_x.get()) { set_error("mdns_spectra_set_continuum: the spectra need variances and a wavelength grid"); return 1; }
	if (s->fixed_scale) { set_error("mdns_spectra_set_continuum: these spectra are in fixed-scale mode (mdns_spectra_set_fixed_scale): no scale to marginalise, no continuum to profile"); return 1; }
	if (s->nx < P) { set_error("mdns_spectra_set_continuum: spectrum 0 has %d channels, fewer than the %d terms", s->nx, P); return 1; }
	const int ldm = model_ld(s->nx);
	// made in locals and installed on success: the former setting stays in force when this call fails
	DeviceBuffer<double> t_buf, fac_buf;
	DeviceBuffer<int> status_buf;
	int status = INT_MAX;
	bool ok = t_buf.make((size_t) ldm) && fac_buf.make((size_t) s->ndata * kContRec + 1) && status_buf.make(1) &&
	          MDNS_HIP(hipMemcpyAsync(status_buf.get(), &status, sizeof(int), hipMemcpyHostToDevice, c->stream));
	double *const d_t = t_buf.get(), *const d_fac = fac_buf.get();
	int *const d_status = status_buf.get();
	if (ok) {
		hipLaunchKernelGGL(k_continuum_t, dim3((ldm + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, (const double *) s->d_x.get(), s->nx, d_t, ldm);
		ok = launched("k_continuum_t");
	}
	if (ok && s->ndata > 0) {
		const int blocks = s->ndata < c->num_cus * 8 ? s->ndata : c->num_cus * 8;
#define CONT_SETUP(PP) hipLaunchKernelGGL((k_continuum_setup<PP>), dim3(blocks), dim3(kBlock), 0, c->stream, (const double *) s->d_y.get(), \
		(const double *) s->d_w.get(), s->ld, s->nx, (const double *) d_t, s->ndata, d_fac, d_status)
		if (P == 1) CONT_SETUP(1); else if (P == 2) CONT_SETUP(2); else if (P == 3) CONT_SETUP(3); else CONT_SETUP(4);
#undef CONT_SETUP
		ok = launched("k_continuum_setup");
	}
	ok = ok && MDNS_HIP(hipMemcpyAsync(&status, d_status, sizeof(int), hipMemcpyDeviceToHost, c->stream));
	ok = MDNS_HIP(hipStreamSynchronize(c->stream)) && ok;
	if (ok && status != INT_MAX) {
		set_error("mdns_spectra_set_continuum: spectrum %d has fewer than %d channels with weight", status, P);
		ok = false;
	}
	if (!ok) return 1;
	s->d_ct = std::move(t_buf); s->d_cfac = std::move(fac_buf);
	s->continuum = P;
	return 0;
}

extern "C" int mdns_muse_continuum_fit_batch_dev(mdns_spectra *s, const double *d_ypred, int B, const int *d_row_ids, int M,
                                                 double *d_Lout, double *d_scale_out, double *d_coef_out)
{
	if (!ctx()) return 1;
	if (!s) { set_error("mdns_muse_continuum_fit_batch_dev: null spectra handle"); return 1; }
	if (B < 0 || M < 0 || M > s->ndata) { set_error("mdns_muse_continuum_fit_batch_dev: bad sizes B=%d M=%d (ndata=%d)", B, M, s->ndata); return 1; }
	if (s->continuum < 1) { set_error("mdns_muse_continuum_fit_batch_dev: no continuum is set on these spectra (mdns_spectra_set_continuum)"); return 1; }
	if (B == 0 || M == 0) return 0;
	if (!d_ypred || !d_Lout) { set_error("mdns_muse_continuum_fit_batch_dev: null argument"); return 1; }
	int ldc = curve_bins(s);                                              // (rows of n_in bins with a response: folded to rows of nx)
	if (!response_fold(s, &d_ypred, &ldc, B)) return 1;
	const int ldm = model_ld(s->nx);
	if (!s->d_model.fit((size_t) B * ldm)) return 1;
	if (!launch_pad_model(d_ypred, s->nx, B, s->d_model.get(), ldm)) return 1;
	return launch_continuum_rows(s, s->d_model.get(), ldm, B, d_row_ids, M, d_Lout, d_scale_out, d_coef_out) ? 0 : 1;
}

extern "C" int mdns_muse_continuum_fit_batch(mdns_spectra *s, const double *ypred, int B, const int *row_ids, int M,
                                             double *Lout, double *scale_out, double *coef_out)
{
	Context *c = ctx();
	if (!c) return 1;
	if (!s) { set_error("mdns_muse_continuum_fit_batch: null spectra handle"); return 1; }
	if (B < 0 || M < 0 || M > s->ndata) { set_error("mdns_muse_continuum_fit_batch: bad sizes B=%d M=%d (ndata=%d)", B, M, s->ndata); return 1; }
	if (s->continuum < 1) { set_error("mdns_muse_continuum_fit_batch: no continuum is set on these spectra (mdns_spectra_set_continuum)"); return 1; }
	if (B == 0 || M == 0) return 0;
	if (!ypred) { set_error("mdns_muse_continuum_fit_batch: null argument"); return 1; }
	if (row_ids) {
		for (int k = 0; k < M; k++)
			if (row_ids[k] < 0 || row_ids[k] >= s->ndata) {
				set_error("mdns_muse_continuum_fit_batch: row_ids[%d]=%d outside [0,%d)", k, row_ids[k], s->ndata);
				return 1;
			}
	}
	const int P = s->continuum;
	const size_t np = (size_t) B * curve_bins(s), n = (size_t) B * M;
	// d_out: L [B][M] | scale [B][M] | coef [B][M][P]
	if (!s->d_params.fit(np) || !s->d_out.fit(n * (2 + P)) || (row_ids && !s->d_rows.fit((size_t) M))) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(s->d_params.get(), ypred, np * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (row_ids && !MDNS_HIP(hipMemcpyAsync(s->d_rows.get(), row_ids, (size_t) M * sizeof(int), hipMemcpyHostToDevice, c->stream))) return 1;
	double *d_L = s->d_out.get(), *d_s = d_L + n, *d_c = d_s + n;
	if (mdns_muse_continuum_fit_batch_dev(s, s->d_params.get(), B, row_ids ? s->d_rows.get() : nullptr, M, d_L,
	                                      scale_out ? d_s : nullptr, coef_out ? d_c : nullptr) != 0) return 1;
	if (Lout && !MDNS_HIP(hipMemcpyAsync(Lout, d_L, n * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	if (scale_out && !MDNS_HIP(hipMemcpyAsync(scale_out, d_s, n * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	if (coef_out && !MDNS_HIP(hipMemcpyAsync(coef_out, d_c, n * P * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
