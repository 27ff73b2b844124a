// Caller-defined models: likelihoods from model CURVES the caller made (include/mdns.h Parts 2, 9, 10, 11), for any
// model.  Four statistics, one tile kernel body: L [B][M] of B candidate curves against M selected spectra.
//
// THE TILE.  One workgroup (four waves) scores S selected spectra x 4 NC candidates: a lane owns NS spectra (S = 64 NS),
// a wave NC candidates, NC x NS sums per lane in registers.  Channels go by in stages of CH; a stage's piece of the
// spectrum rows and of the curves is put into LDS while the next stage's loads are already in flight in registers.  A
// spectrum value is read from LDS once per NC candidates, a curve value -- the same address in all lanes, a broadcast
// -- once per NS spectra.  A wave without a candidate still stages and then idles.
//
// THE SPECTRUM STAGE (RowStage<A, CH, S>).  A statistic reads A arrays of [n_datasets][ld] rows.  A CH/2 consecutive
// threads read one selected row: each ONE 16-byte channel pair of ONE array, so a row costs A x CH x 8 contiguous bytes
// per stage and a sparse selection exactly its own bytes.  The pairs go into A arrays of [CH/2][S + 1] 16-byte slots,
// [channel pair][spectrum].  The one slot more than the spectra is for the banks: a store group of ds_write_b128 is
// eight contiguous lanes -- eight channel pairs of one spectrum in one array --, banks are (address / 4) mod 32, and
// the eight lanes are S + 1 slots = 4 (S + 1) dwords = 4 mod 32 apart: eight times four different banks, no conflict.
// (A separate arrays and not the A values of a channel in one slot: interleaved, the lanes of a group would be a
// multiple of 8 dwords apart and collide in pairs.)  One compile-time switch, EVERY, for k_curve_rows_w alone: CH/2
// threads read a row, each its channel pair of EVERY array -- the same loads, bytes per row and store groups; measured
// beside the common mapping, which that kernel's small shape did not bear.
//   tail   rows are 16-byte aligned and an even number of doubles long, so the pair of an even channel below nx is
//          inside; a pair at or past nx is staged as zero, and .y = 0 where j + 1 >= nx.
//   clamp  a thread whose row index is M or more reads row M - 1 of the selection again; its sums are never stored.
//
// THE CURVE STAGE (CurveStage<T, NCAND, CH>).  [candidate][channel] elements T, thread t bringing channel t mod CH of
// the candidates t / CH, t / CH + 256 / CH, ...: all threads where NCAND x CH >= 256, the first of them otherwise.
// A store group is contiguous bytes of one candidate.  Zero past candidate B and (unless the rows are whole stages
// long) past channel nx.
//
// Per (curve, spectrum) pair every statistic is ONE chain over the channels in ascending order from acc = +0, so the
// bits of a pair do not depend on B, M, where either sits in its batch, ldc, the grid split or the entry point.
// Nothing is validated: a non-finite curve value propagates as IEEE.
//
// k_curve_rows    fixed noise (Part 2; what K1 computes from (A, mu, sig)):  L = -0.5 sum_j ((c_j - y_j) / noise)^2
//     d = c - y;  acc = fma(d, d, acc);                                        L = acc * scale,  scale = -0.5 / noise^2
//   Channels past the last one: fma(0, 0, acc) = acc.  A = 1, CH = 32, 128 x 32 tile (NC = 8, NS = 2).
//   LDS 16 x 129 x 16 B + 32 x 32 x 8 B = 41 216 B.
//
// k_curve_rows_w  fixed-scale chi^2 with per-pixel weights w = 1 / v (Part 9; s->d_w, 0 for a masked pixel):
//     d = c - y;  t = w * d (a rounded product);  acc = fma(t, d, acc);        L = -0.5 * acc
//   Channels past the last one are y = w = c = 0.  A masked pixel -- w = 0 and a finite y (like.WeightedSpectra sees to
//   both) -- gives t = +-0 and fma(+-0, d, acc) = acc for every finite d, bit for bit (acc = +0 stays +0): the kernel
//   does not look for masks.  A = 2 (y, w), CH = 32, 128 x 32 tile.  LDS 2 x 16 x 129 x 16 B + 8 KB = 74 240 B.
//
// k_curve_rows_p  Poisson likelihood of counts (Part 10): n = s->d_y, exposures e = s->d_e, K = s->d_koff the host's
//   sum n (1 + log e - log n), -C/2 of the C statistic:  L = sum_j (n_j log max(c_j, tiny) - e_j c_j) + K, tiny = DBL_MIN
//     acc = fma(n, lc, acc);  acc = fma(-e, c', acc);                          L = acc + K
//   k_curve_log stages the curves first, [B][ldc] -> pairs {lc, c'} [B][ldp] (ldp = nx rounded up to a whole stage):
//   c' = c for c >= 0 (-0 included) and NaN otherwise, lc = log(fmax(c', tiny)) by the device library's fp64 log,
//   {0, 0} behind channel nx: one log per candidate and channel, never one per pair.  Channels past the last one are
//   n = e = 0: fma(+-0, 0, acc) = acc.  A masked pixel is n = e = 0 (mdns_spectra_set_counts zeroes n where e = 0): a
//   deleted channel for every finite lc and c', bit for bit.  c = +-0 gives lc = log(tiny), about -708.4: nothing
//   where n = 0, finite and ordered where n > 0.  A negative or NaN curve value is c' = NaN, and fma(-e, NaN, acc) is
//   NaN even at e = 0: NaN for every spectrum, which the accept test rejects.  +inf is not validated.
//   A = 2 (n, e), CH = 16, 128 x 32 tile, curve elements the 16-byte pairs.  LDS 2 x 8 x 129 x 16 B + 32 x 16 x 16 B =
//   41 216 B.  The curve broadcast -- two 16-byte reads per candidate and channel pair -- weighs most here.
//
// k_curve_rows_b  W statistic of counts with a background spectrum each (Part 11): n, e as above; b = s->d_b the
//   background region's counts, g = s->d_g its exposures (area ratio included), Kw = s->d_kw the host's offsets.  The
//   background rate f of a pixel is profiled out of the joint Poisson likelihood in closed form, per (candidate,
//   spectrum, channel):
//     wstat_pixel  T = e + g;  N = n + b;  Q = 4 (T b);  T2 = 2 T, or 1 where T == 0;  b2 = 2 b
//     wstat_rate   a = fma(-T, c', N);  d = sqrt(fma(a, a, Q c'));
//                  f = (a + d) / T2 where a >= 0,  f = (b2 c') / (d - a) where not   (the branch that does not cancel)
//     wstat_term   s = c' + f
//                  acc = fma(n, log(fmax(s, tiny)), acc);  acc = fma(b, log(fmax(f, tiny)), acc);
//                  acc = fma(-e, s, acc);                  acc = fma(-g, f, acc)     L = acc + Kw
//   with the device library's fp64 log, sqrt and division; c' as above, made in the curve fetch (no pre-pass: f depends
//   on all three indices).  The per-pixel values are made in registers from the four staged ones.  A masked pixel is
//   n = e = b = g = 0 (mdns_spectra_set_background zeroes all four where any side is masked), and a channel past the
//   last one is staged the same with c' = 0: T = N = Q = b2 = 0 and T2 = 1, so a = +0, d = 0, f = 0 / 1 = 0 -- no
//   0/0 --, s = c', and the four fma add +-0 for every finite c' >= 0: a deleted channel, bit for bit.  The guard is T2,
//   a per-pixel value; no candidate is tested.  A NaN c' makes a, d, f, s NaN; fmax drops it from the logarithms,
//   fma(-e, NaN, acc) is NaN even at e = 0: NaN for every spectrum of that candidate.  c' = +-0 with n > 0, b = 0:
//   a = N, f = 2 N / (2 T) = n / T.
//   A pair and channel costs two inlined logarithms, a square root and a division (DESIGN section 4 has the count), so
//   neither LDS nor loads bound it and the tile is as small as the staging allows, which spreads a chunk of a few
//   thousand pairs over the chip: A = 4, CH = 16, 64 x 4 tile (NC = NS = 1), the channel-pair loop not unrolled.
//   LDS 4 x 8 x 65 x 16 B + 4 x 16 x 8 B = 33 792 B.
// k_curve_background  the same wstat_pixel and wstat_rate, elementwise: f [B][M][nx] (mdns_curve_background_batch).
#include "mdns_internal.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace mdns {

// ---- staging (file header) ----
template <int A, int CH, int S, bool EVERY> struct RowStage {
	// EVERY: CH/2 threads read a row, each its channel pair of every array (k_curve_rows_w alone: DESIGN section 4)
	static constexpr int kPairs = CH / 2, kLanes = (EVERY ? 1 : A) * kPairs, kStep = 256 / kLanes, kRows = S / kStep;
	static constexpr int kLoads = (EVERY ? A : 1) * kRows;
	static_assert(CH % 2 == 0 && 256 % kLanes == 0 && S % kStep == 0, "whole rows per pass, whole passes per tile");
	typedef double2 Lds[A][kPairs][S + 1];
	int cp, which, rsub;                                  // this thread's channel pair and array, of rows rsub, rsub + kStep, ...
	const double *src[kLoads];
	double2 v[kLoads];

	template <class Stat> __device__ __forceinline__ RowStage(const Stat &stat, int ld, const int *__restrict__ rows, int M, int k0)
	    : cp(threadIdx.x % kPairs), which(EVERY ? 0 : threadIdx.x / kPairs % A), rsub(threadIdx.x / kLanes)
	{
#pragma unroll
		for (int i = 0; i < kRows; i++) {
			const int k = k0 + rsub + kStep * i;
			const int kk = k < M ? k : M - 1;                                 // (past the selection: its last row again, never stored)
			const size_t at = (size_t) (rows ? rows[kk] : kk) * ld + 2 * cp;
#pragma unroll
			for (int a = 0; a < kLoads / kRows; a++) src[a * kRows + i] = stat.array(which + a) + at;
		}
	}
	// (all loads of a stage under one test and the tail's .y = 0 in a block of its own, which only the last stage enters:
	// the loads are issued together and nothing waits for them before the store, one stage of arithmetic later)
	__device__ __forceinline__ void fetch(int j0, int nx)
	{
		const int j = j0 + 2 * cp;
		if (j < nx) {
#pragma unroll
			for (int i = 0; i < kLoads; i++) v[i] = *reinterpret_cast<const double2 *>(src[i] + j0);
		} else {
#pragma unroll
			for (int i = 0; i < kLoads; i++) v[i] = make_double2(0.0, 0.0);
		}
		if (j + 1 >= nx) {
#pragma unroll
			for (int i = 0; i < kLoads; i++) v[i].y = 0.0;
		}
	}
	__device__ __forceinline__ void store(Lds &px) const
	{
#pragma unroll
		for (int i = 0; i < kLoads; i++) px[which + i / kRows][cp][rsub + kStep * (i % kRows)] = v[i];
	}
};

template <typename T, int NCAND, int CH> struct CurveStage {
	static constexpr int kStep = 256 / CH, kLoads = NCAND > kStep ? NCAND / kStep : 1;
	static_assert(256 % CH == 0 && (NCAND % kStep == 0 || NCAND < kStep), "whole candidates per pass");
	typedef T Lds[NCAND][CH];
	int cch, crow, left;                                  // this thread's channel, of candidates crow, crow + kStep, ... below `left`
	const T *src;
	size_t pass;
	T v[kLoads];

	__device__ __forceinline__ CurveStage(const T *__restrict__ curves, int ldc, int B, int b0)
	    : cch(threadIdx.x % CH), crow(threadIdx.x / CH), left(NCAND >= kStep || crow < NCAND ? B - b0 - crow : 0),
	      src(curves + (size_t) (b0 + crow) * ldc + cch), pass((size_t) kStep * ldc) {}
	template <class Stat> __device__ __forceinline__ void fetch(int j0, int nx)
	{
#pragma unroll
		for (int i = 0; i < kLoads; i++) {
			T c = T();
			if (kStep * i < left && (Stat::kWholeStages || j0 + cch < nx)) c = Stat::curve(src[i * pass + j0]);
			v[i] = c;
		}
	}
	__device__ __forceinline__ void store(Lds &cs) const
	{
		if (NCAND < kStep && crow >= NCAND) return;
#pragma unroll
		for (int i = 0; i < kLoads; i++) cs[crow + kStep * i][cch] = v[i];
	}
};

// ---- the statistics (file header): the arrays [ndata][ld] and the stage length, the curve element, one channel's step
// of a chain, and the finish from what it needs of the spectrum's row ----
// array `which` of a statistic's.  By value: a choice among the members themselves is one load through a chosen address,
// which keeps the struct in memory
template <typename... P> __device__ __forceinline__ const double *pick(int which, const double *first, P... rest)
{
	if constexpr (sizeof...(rest) == 0) return first;
	else return which == 0 ? first : pick(which - 1, rest...);
}

struct StatNoise {
	static constexpr int A = 1, CH = 32;
	static constexpr bool kWholeStages = false, kEveryArray = false;
	typedef double Curve;
	const double *y;
	double scale;
	__device__ __forceinline__ const double *array(int) const { return y; }
	static __device__ __forceinline__ double curve(double c) { return c; }
	static __device__ __forceinline__ double step(const double (&p)[A], double c, double acc) { const double d = c - p[0]; return fma(d, d, acc); }
	__device__ __forceinline__ double of_row(int) const { return scale; }
	static __device__ __forceinline__ double finish(double acc, double scale) { return acc * scale; }
};

struct StatChi2 {
	static constexpr int A = 2, CH = 32;                  // y, w
	static constexpr bool kWholeStages = false, kEveryArray = true;
	typedef double Curve;
	const double *y, *w;
	__device__ __forceinline__ const double *array(int which) const { return pick(which, y, w); }
	static __device__ __forceinline__ double curve(double c) { return c; }
	static __device__ __forceinline__ double step(const double (&p)[A], double c, double acc) { const double d = c - p[0]; return fma(__dmul_rn(p[1], d), d, acc); }
	__device__ __forceinline__ double of_row(int) const { return -0.5; }
	static __device__ __forceinline__ double finish(double acc, double half) { return half * acc; }
};

struct StatPoisson {
	static constexpr int A = 2, CH = 16;                  // n, e
	static constexpr bool kWholeStages = true, kEveryArray = false;            // (k_curve_log's rows)
	typedef double2 Curve;                                // {lc, c'}
	const double *n, *e, *K;
	__device__ __forceinline__ const double *array(int which) const { return pick(which, n, e); }
	static __device__ __forceinline__ double2 curve(double2 c) { return c; }
	static __device__ __forceinline__ double step(const double (&p)[A], double2 c, double acc) { return fma(-p[1], c.y, fma(p[0], c.x, acc)); }
	__device__ __forceinline__ double of_row(int row) const { return K[row]; }
	static __device__ __forceinline__ double finish(double acc, double K) { return acc + K; }
};

// what a pixel contributes to every candidate's term: the four staged values and what follows from them alone
struct WPixel { double n, e, b, g, T, N, Q, T2, b2; };

__device__ __forceinline__ WPixel wstat_pixel(double n, double e, double b, double g)
{
	WPixel p;
	p.n = n; p.e = e; p.b = b; p.g = g;
	p.T = e + g;
	p.N = n + b;
	p.Q = 4.0 * (p.T * b);
	p.T2 = p.T == 0.0 ? 1.0 : 2.0 * p.T;                                  // (a masked pixel: f = 0 / 1, never 0 / 0)
	p.b2 = 2.0 * b;
	return p;
}

// the profiled background rate f of a pixel under the source rate c (c >= 0, or NaN): the branch that does not cancel
__device__ __forceinline__ double wstat_rate(const WPixel &p, double c)
{
	const double a = fma(-p.T, c, p.N);
	const double d = sqrt(fma(a, a, p.Q * c));
	const bool up = a >= 0.0;
	const double num = up ? a + d : p.b2 * c, den = up ? p.T2 : d - a;
	return num / den;
}

__device__ __forceinline__ double wstat_term(const WPixel &p, double c, double acc)
{
	const double f = wstat_rate(p, c);
	const double s = c + f;
	acc = fma(p.n, log(fmax(s, DBL_MIN)), acc);
	acc = fma(p.b, log(fmax(f, DBL_MIN)), acc);
	acc = fma(-p.e, s, acc);
	return fma(-p.g, f, acc);
}

struct StatWstat {
	static constexpr int A = 4, CH = 16;                  // n, e, b, g
	static constexpr bool kWholeStages = false, kEveryArray = false;
	typedef double Curve;                                 // c'
	const double *n, *e, *b, *g, *Kw;
	__device__ __forceinline__ const double *array(int which) const { return pick(which, n, e, b, g); }
	static __device__ __forceinline__ double curve(double c) { return c >= 0.0 ? c : (double) NAN; }
	static __device__ __forceinline__ double step(const double (&p)[A], double c, double acc) { return wstat_term(wstat_pixel(p[0], p[1], p[2], p[3]), c, acc); }
	__device__ __forceinline__ double of_row(int row) const { return Kw[row]; }
	static __device__ __forceinline__ double finish(double acc, double Kw) { return acc + Kw; }
};

// ---- the tile (file header): NC candidates per wave x NS spectra per lane, the channel-pair loop unrolled UNROLL times ----
static constexpr int kCurveNC = 8, kCurveNS = 2;          // k_curve_rows, _w, _p: 128 spectra x 32 candidates
static constexpr int kBgNC = 1, kBgNS = 1;                // k_curve_rows_b: 64 x 4

template <typename T> struct alignas(16) ChannelPair { T lo, hi; };

template <class Stat, int NC, int NS, int UNROLL>
__device__ __forceinline__ void curve_tile(const Stat &stat, int ld, int nx,
                                           const typename Stat::Curve *__restrict__ curves, int ldc, int B,
                                           const int *__restrict__ rows, int M, double *__restrict__ out)
{
	constexpr int A = Stat::A, CH = Stat::CH, S = 64 * NS, NCAND = 4 * NC;
	typedef typename Stat::Curve Curve;
	typedef RowStage<A, CH, S, Stat::kEveryArray> Rows;
	typedef CurveStage<Curve, NCAND, CH> Curves;
	__shared__ __attribute__((aligned(16))) typename Rows::Lds px;
	__shared__ __attribute__((aligned(16))) typename Curves::Lds cs;
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int k0 = blockIdx.x * S, b0 = blockIdx.y * NCAND;
	Rows rs(stat, ld, rows, M, k0);
	Curves cv(curves, ldc, B, b0);
	double acc[NC][NS];
#pragma unroll
	for (int c = 0; c < NC; c++)
#pragma unroll
		for (int s = 0; s < NS; s++) acc[c][s] = 0.0;
	const bool working = b0 + wave * NC < B;                                  // wave-uniform; an idle wave still stages
	rs.fetch(0, nx);
	cv.template fetch<Stat>(0, nx);
	for (int j0 = 0; j0 < nx; j0 += CH) {
		rs.store(px);
		cv.store(cs);
		__syncthreads();
		if (j0 + CH < nx) {
			rs.fetch(j0 + CH, nx);
			cv.template fetch<Stat>(j0 + CH, nx);
		}
		if (working) {
#pragma unroll UNROLL
			for (int jp = 0; jp < CH / 2; jp++) {
				double lo[NS][A], hi[NS][A];
#pragma unroll
				for (int a = 0; a < A; a++)
#pragma unroll
					for (int s = 0; s < NS; s++) {
						const double2 p = px[a][jp][lane + 64 * s];
						lo[s][a] = p.x; hi[s][a] = p.y;
					}
#pragma unroll
				for (int c = 0; c < NC; c++) {
					const ChannelPair<Curve> m = *reinterpret_cast<const ChannelPair<Curve> *>(&cs[wave * NC + c][2 * jp]);
#pragma unroll
					for (int s = 0; s < NS; s++) acc[c][s] = Stat::step(hi[s], m.hi, Stat::step(lo[s], m.lo, acc[c][s]));
				}
			}
		}
		__syncthreads();
	}
	if (!working) return;
	double of_row[NS];
#pragma unroll
	for (int s = 0; s < NS; s++) {
		const int k = k0 + lane + 64 * s;
		of_row[s] = k < M ? stat.of_row(rows ? rows[k] : k) : 0.0;
	}
#pragma unroll
	for (int c = 0; c < NC; c++) {
		const int b = b0 + wave * NC + c;
		if (b >= B) break;
#pragma unroll
		for (int s = 0; s < NS; s++) {
			const int k = k0 + lane + 64 * s;
			if (k < M) out[(size_t) b * M + k] = Stat::finish(acc[c][s], of_row[s]);
		}
	}
}

__global__ __launch_bounds__(256) void k_curve_rows(
    const double *__restrict__ Y, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double scale, double *__restrict__ out)
{
	curve_tile<StatNoise, kCurveNC, kCurveNS, 4>(StatNoise{Y, scale}, ld, nx, curves, ldc, B, rows, M, out);
}

__global__ __launch_bounds__(256) void k_curve_rows_w(
    const double *__restrict__ Y, const double *__restrict__ W, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double *__restrict__ out)
{
	curve_tile<StatChi2, kCurveNC, kCurveNS, 4>(StatChi2{Y, W}, ld, nx, curves, ldc, B, rows, M, out);
}

// row stride, in {lc, c'} pairs, of the block k_curve_log stages: whole stages, so that k_curve_rows_p tests no channel
static inline int count_ld(int nx) { return (nx + StatPoisson::CH - 1) / StatPoisson::CH * StatPoisson::CH; }

// curves [B][ldc] -> staged [B][ldp] pairs {lc, c'}: c' = c for c >= 0 (and -0), NaN otherwise; lc = log(fmax(c', tiny))
// (fmax drops the NaN: lc is finite, the NaN travels in c'); {0, 0} behind channel nx
__global__ __launch_bounds__(256) void k_curve_log(const double *__restrict__ curves, int ldc, int nx, double2 *__restrict__ staged, int ldp)
{
	const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
	if (j >= ldp) return;
	double2 p = make_double2(0.0, 0.0);
	if (j < nx) {
		const double c = curves[(size_t) b * ldc + j];
		p.y = c >= 0.0 ? c : (double) NAN;
		p.x = log(fmax(p.y, DBL_MIN));
	}
	staged[(size_t) b * ldp + j] = p;
}

__global__ __launch_bounds__(256) void k_curve_rows_p(
    const double *__restrict__ Y, const double *__restrict__ E, const double *__restrict__ K, int ld, int nx,
    const double2 *__restrict__ P, int ldp, int B, const int *__restrict__ rows, int M, double *__restrict__ out)
{
	curve_tile<StatPoisson, kCurveNC, kCurveNS, 4>(StatPoisson{Y, E, K}, ld, nx, P, ldp, B, rows, M, out);
}

__global__ __launch_bounds__(256) void k_curve_rows_b(
    const double *__restrict__ Y, const double *__restrict__ E, const double *__restrict__ Bc, const double *__restrict__ G,
    const double *__restrict__ Kw, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double *__restrict__ out)
{
	curve_tile<StatWstat, kBgNC, kBgNS, 1>(StatWstat{Y, E, Bc, G, Kw}, ld, nx, curves, ldc, B, rows, M, out);
}

// y[i] = 0 where e[i] == 0, over the whole [ndata][ld] block (mdns_spectra_set_counts: a masked pixel holds no counts)
__global__ __launch_bounds__(256) void k_counts_mask(double *__restrict__ y, const double *__restrict__ e, size_t n)
{
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if (i < n && e[i] == 0.0) y[i] = 0.0;
}

// f [B][M][nx]: the profiled background rate of every (candidate, selected spectrum, channel), by the device functions
// k_curve_rows_b scores with; 0 at a masked pixel
__global__ __launch_bounds__(256) void k_curve_background(
    const double *__restrict__ Y, const double *__restrict__ E, const double *__restrict__ Bc, const double *__restrict__ G,
    int ld, int nx, const double *__restrict__ curves, int ldc, const int *__restrict__ rows, int M, double *__restrict__ out)
{
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if (i >= (size_t) M * nx) return;
	const int k = (int) (i / nx), j = (int) (i % nx), b = blockIdx.y;
	const size_t at = (size_t) (rows ? rows[k] : k) * ld + j;
	const double c = curves[(size_t) b * ldc + j];
	out[(size_t) b * M * nx + i] = wstat_rate(wstat_pixel(Y[at], E[at], Bc[at], G[at]), c >= 0.0 ? c : (double) NAN);
}

// y = e = b = g = 0 where e == 0 or g == 0, over the whole [ndata][ld] blocks (mdns_spectra_set_background: a pixel
// masked on either side is masked on both)
__global__ __launch_bounds__(256) void k_background_mask(double *__restrict__ y, double *__restrict__ e, double *__restrict__ b,
                                                         double *__restrict__ g, size_t n)
{
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if (i < n && (e[i] == 0.0 || g[i] == 0.0)) y[i] = e[i] = b[i] = g[i] = 0.0;
}

// curves [B][ldc] -> templates [B][ldm] as the K2 row kernels take them: zero behind channel nx
__global__ __launch_bounds__(256) void k_curve_pad(const double *__restrict__ curves, int ldc, int nx, double *__restrict__ model, int ldm)
{
	const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
	if (j < ldm) model[(size_t) b * ldm + j] = j < nx ? curves[(size_t) b * ldc + j] : 0.0;
}

CurveStat curve_stat(const mdns_spectra *s)
{
	if (s->background) return kCurveWstat;
	if (s->counts) return kCurvePoisson;
	if (s->fixed_scale) return kCurveChi2;
	return s->d_w.get() ? kCurveMarginal : kCurveNoise;
}

bool launch_curve(CurveStat stat, mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                  const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0) return true;
	const int nc = stat == kCurveWstat ? kBgNC : kCurveNC, ns = stat == kCurveWstat ? kBgNS : kCurveNS;
	const dim3 grid((M + 64 * ns - 1) / (64 * ns), (B + 4 * nc - 1) / (4 * nc)), block(256);
	const double *y = s->d_y.get(), *e = s->d_e.get();
	switch (stat) {
	case kCurveNoise:
		hipLaunchKernelGGL(k_curve_rows, grid, block, 0, c->stream, y, s->ld, s->nx, d_curves, ldc, B, d_rows, M,
		                   -0.5 / (noise_level * noise_level), d_out);
		return launched("k_curve_rows");
	case kCurveChi2:
		hipLaunchKernelGGL(k_curve_rows_w, grid, block, 0, c->stream, y, (const double *) s->d_w.get(), s->ld, s->nx, d_curves, ldc, B,
		                   d_rows, M, d_out);
		return launched("k_curve_rows_w");
	case kCurvePoisson: {
		const int ldp = count_ld(s->nx);
		if (!ensure_model(s, (size_t) B * ldp * 2)) return false;
		double2 *staged = reinterpret_cast<double2 *>(s->d_model.get());
		hipLaunchKernelGGL(k_curve_log, dim3((ldp + 255) / 256, B), block, 0, c->stream, d_curves, ldc, s->nx, staged, ldp);
		if (!launched("k_curve_log")) return false;
		hipLaunchKernelGGL(k_curve_rows_p, grid, block, 0, c->stream, y, e, (const double *) s->d_koff.get(), s->ld, s->nx,
		                   (const double2 *) staged, ldp, B, d_rows, M, d_out);
		return launched("k_curve_rows_p");
	}
	case kCurveWstat:
		hipLaunchKernelGGL(k_curve_rows_b, grid, block, 0, c->stream, y, e, (const double *) s->d_b.get(), (const double *) s->d_g.get(),
		                   (const double *) s->d_kw.get(), s->ld, s->nx, d_curves, ldc, B, d_rows, M, d_out);
		return launched("k_curve_rows_b");
	case kCurveMarginal:
		break;
	}
	set_error("launch_curve: the scale-marginalised likelihood has no curve kernel");
	return false;
}

bool launch_curve_background(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0 || s->nx <= 0) return true;
	const size_t per = (size_t) M * s->nx;
	for (int lo = 0; lo < B; lo += 65535) {                                   // (the candidate is the grid's y)
		const int nb = B - lo < 65535 ? B - lo : 65535;
		hipLaunchKernelGGL(k_curve_background, dim3((unsigned) ((per + 255) / 256), nb), dim3(256), 0, c->stream,
		                   (const double *) s->d_y.get(), (const double *) s->d_e.get(), (const double *) s->d_b.get(),
		                   (const double *) s->d_g.get(), s->ld, s->nx, d_curves + (size_t) lo * ldc, ldc, d_rows, M, d_out + lo * per);
		if (!launched("k_curve_background")) return false;
	}
	return true;
}

bool launch_curve_pad(const double *d_curves, int ldc, int nx, int B, double *d_model, int ldm)
{
	Context *c = ctx();
	if (B <= 0) return true;
	hipLaunchKernelGGL(k_curve_pad, dim3((ldm + 255) / 256, B), dim3(256), 0, c->stream, d_curves, ldc, nx, d_model, ldm);
	return launched("k_curve_pad");
}

}  // namespace mdns

using namespace mdns;

// what the device entry points check first; 1: refused, 0: go on, -1: nothing to score.  stat: the likelihood, for what
// it asks of the handle
static int curve_batch_check(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                             const double *d_Lout, CurveStat stat, const char *who)
{
	if (!ctx()) return 1;
	if (!s) { set_error("%s: null spectra handle", who); return 1; }
	if (B < 0 || M < 0 || M > s->ndata || s->nx < 1 || ldc < curve_bins(s) || (!d_row_ids && M != s->ndata && M != 0)) {
		if (s->response) set_error("%s: bad sizes B=%d M=%d (ndata=%d) ldc=%d (n_in=%d of the response)", who, B, M, s->ndata, ldc, curve_bins(s));
		else set_error("%s: bad sizes B=%d M=%d (ndata=%d) ldc=%d (nx=%d)", who, B, M, s->ndata, ldc, s->nx);
		return 1;
	}
	if (stat == kCurveChi2 && !s->d_w.get()) { set_error("%s: spectra were created without variances", who); return 1; }
	if (stat == kCurvePoisson && !s->counts) { set_error("%s: spectra are not in counts mode (mdns_spectra_set_counts)", who); return 1; }
	if (stat == kCurveWstat && !s->background) { set_error("%s: spectra have no background (mdns_spectra_set_background)", who); return 1; }
	if (B == 0 || M == 0) return -1;
	if (!d_curves || !d_Lout) { set_error("%s: null argument", who); return 1; }
	return 0;
}

static int curve_batch_dev(CurveStat stat, mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                           const int *d_row_ids, int M, double *d_Lout, const char *who)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_Lout, stat, who);
	if (rc != 0) return rc > 0;
	if (!response_fold(s, &d_curves, &ldc, B)) return 1;
	return launch_curve(stat, s, d_curves, ldc, B, noise_level, d_row_ids, M, d_Lout) ? 0 : 1;
}

extern "C" int mdns_curve_loglike_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                                            const int *d_row_ids, int M, double *d_Lout)
{
	return curve_batch_dev(kCurveNoise, s, d_curves, ldc, B, noise_level, d_row_ids, M, d_Lout, "mdns_curve_loglike_batch_dev");
}

extern "C" int mdns_curve_chi2_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                         double *d_Lout)
{
	return curve_batch_dev(kCurveChi2, s, d_curves, ldc, B, 0, d_row_ids, M, d_Lout, "mdns_curve_chi2_batch_dev");
}

extern "C" int mdns_curve_poisson_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                            double *d_Lout)
{
	return curve_batch_dev(kCurvePoisson, s, d_curves, ldc, B, 0, d_row_ids, M, d_Lout, "mdns_curve_poisson_batch_dev");
}

extern "C" int mdns_curve_wstat_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                          double *d_Lout)
{
	return curve_batch_dev(kCurveWstat, s, d_curves, ldc, B, 0, d_row_ids, M, d_Lout, "mdns_curve_wstat_batch_dev");
}

extern "C" int mdns_spectra_fixed_scale(const mdns_spectra *s) { return s ? s->fixed_scale : -1; }

extern "C" int mdns_spectra_set_fixed_scale(mdns_spectra *s, int on)
{
	if (!s) { set_error("mdns_spectra_set_fixed_scale: null spectra handle"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_fixed_scale: a joint state exists on these spectra (set the mode first)"); return 1; }
	if (on && !s->d_w.get()) { set_error("mdns_spectra_set_fixed_scale: spectra were created without variances"); return 1; }
	if (on && s->continuum > 0) {
		set_error("mdns_spectra_set_fixed_scale: a continuum of %d terms is set on these spectra (it belongs to the scale-marginalised likelihood)", s->continuum);
		return 1;
	}
	s->fixed_scale = on ? 1 : 0;
	return 0;
}

// ---- counts and their background: what both setters do ----
// a host block [ndata][nx] (nullptr: `fill` everywhere) as device rows the way the kernels read them: [ndata][ld] with
// the slack of d_y, zero behind channel nx.  Synchronised: the host copy may go
static bool device_rows(Context *c, const mdns_spectra *s, const double *block, double fill, DeviceBuffer<double> &d_rows)
{
	const size_t elems = (size_t) s->ndata * s->ld + 2;
	std::vector<double> padded(elems, 0.0);
	for (int k = 0; k < s->ndata; k++)
		for (int j = 0; j < s->nx; j++) padded[(size_t) k * s->ld + j] = block ? block[(size_t) k * s->nx + j] : fill;
	return d_rows.make(elems) && MDNS_HIP(hipMemcpyAsync(d_rows.get(), padded.data(), elems * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	       MDNS_HIP(hipStreamSynchronize(c->stream));
}

// the per-spectrum offsets [ndata] (nullptr: zeros) on the device, never an empty block
static bool device_offsets(Context *c, const mdns_spectra *s, const double *offsets, DeviceBuffer<double> &d_off)
{
	std::vector<double> off((size_t) (s->ndata > 0 ? s->ndata : 1), 0.0);
	if (offsets) for (int k = 0; k < s->ndata; k++) off[k] = offsets[k];
	return d_off.make(off.size()) && MDNS_HIP(hipMemcpyAsync(d_off.get(), off.data(), off.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	       MDNS_HIP(hipStreamSynchronize(c->stream));
}

// after a mask kernel changed d_y: what the handle keeps derived from y follows (the Gaussian batch functions then score
// the y that is on the handle)
static bool spectra_changed(Context *c, mdns_spectra *s)
{
	bool ok = true;
	if (s->d_yT.get()) ok = launch_tile_columns(s->d_y.get(), s->ld, s->ndata, s->nx, nullptr, s->d_yT.get());
	if (ok && s->d_ysq.get()) ok = launch_row_sumsq(s->d_y.get(), s->ld, s->nx, s->ndata, s->d_ysq.get());
	if (!ok || !MDNS_HIP(hipStreamSynchronize(c->stream))) return false;
	s->d_yG.release();                                            // (made again from the new y on first use)
	return true;
}

extern "C" int mdns_spectra_counts(const mdns_spectra *s) { return s ? s->counts : -1; }

extern "C" int mdns_spectra_set_counts(mdns_spectra *s, const double *exposure, const double *offsets)
{
	if (!s) { set_error("mdns_spectra_set_counts: null spectra handle"); return 1; }
	Context *c = ctx();
	if (!c) return 1;
	if (s->d_w.get()) { set_error("mdns_spectra_set_counts: spectra were created with variances (counts carry none: their noise is Poisson)"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_counts: a joint state exists on these spectra (set the mode first)"); return 1; }
	if (s->background) { set_error("mdns_spectra_set_counts: these spectra have a background (its masks and offsets belong to the exposures that are set)"); return 1; }
	const int ndata = s->ndata, nx = s->nx;
	// the host copy is looked at before anything is uploaded
	bool any_zero = false;
	if (exposure) {
		for (int k = 0; k < ndata; k++)
			for (int j = 0; j < nx; j++) {
				const double e = exposure[(size_t) k * nx + j];
				if (!(e >= 0.0) || std::isinf(e)) {
					set_error("mdns_spectra_set_counts: exposure[%d][%d] = %g: exposures must be finite and >= 0 (0 masks a pixel)", k, j, e);
					return 1;
				}
				any_zero = any_zero || e == 0.0;
			}
	}
	// made in locals and installed on success: the handle stays as it was when this call fails
	DeviceBuffer<double> d_e, d_koff;
	if (!device_rows(c, s, exposure, 1.0, d_e) || !device_offsets(c, s, offsets, d_koff)) return 1;
	if (any_zero && ndata > 0 && nx > 0) {
		// a masked pixel holds no counts
		const size_t elems = (size_t) ndata * s->ld + 2;
		hipLaunchKernelGGL(k_counts_mask, dim3((unsigned) ((elems + 255) / 256)), dim3(256), 0, c->stream, s->d_y.get(), (const double *) d_e.get(), elems);
		if (!launched("k_counts_mask") || !spectra_changed(c, s)) return 1;
	}
	s->d_e = std::move(d_e);
	s->d_koff = std::move(d_koff);
	s->counts = 1;
	return 0;
}

// ---- counts with a background (mdns.h Part 11) ----
extern "C" int mdns_curve_background_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                               double *d_fout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_fout, kCurveWstat, "mdns_curve_background_batch_dev");
	if (rc != 0) return rc > 0;
	if (!response_fold(s, &d_curves, &ldc, B)) return 1;
	return launch_curve_background(s, d_curves, ldc, B, d_row_ids, M, d_fout) ? 0 : 1;
}

extern "C" int mdns_curve_background_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *fout)
{
	Context *c = ctx();
	const int rc = curve_batch_check(s, curves, s ? curve_bins(s) : 0, B, row_ids, M, fout, kCurveWstat, "mdns_curve_background_batch");
	if (rc != 0) return rc > 0;
	if (row_ids) {
		for (int k = 0; k < M; k++)
			if (row_ids[k] < 0 || row_ids[k] >= s->ndata) {
				set_error("mdns_curve_background_batch: row_ids[%d]=%d outside [0,%d)", k, row_ids[k], s->ndata);
				return 1;
			}
	}
	const size_t np = (size_t) B * curve_bins(s), no = (size_t) B * M * s->nx;
	if (!s->d_params.fit(np) || !s->d_out.fit(no) || (row_ids && !s->d_rows.fit((size_t) M))) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(s->d_params.get(), curves, np * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (row_ids && !MDNS_HIP(hipMemcpyAsync(s->d_rows.get(), row_ids, (size_t) M * sizeof(int), hipMemcpyHostToDevice, c->stream))) return 1;
	const double *d_curves = s->d_params.get();
	int ldc = curve_bins(s);
	if (!response_fold(s, &d_curves, &ldc, B)) return 1;
	if (!launch_curve_background(s, d_curves, ldc, B, row_ids ? s->d_rows.get() : nullptr, M, s->d_out.get())) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(fout, s->d_out.get(), no * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}

extern "C" int mdns_spectra_background(const mdns_spectra *s) { return s ? s->background : -1; }

extern "C" int mdns_spectra_set_background(mdns_spectra *s, const double *bkg_counts, const double *bkg_exposure, const double *offsets)
{
	if (!s) { set_error("mdns_spectra_set_background: null spectra handle"); return 1; }
	Context *c = ctx();
	if (!c) return 1;
	if (!s->counts) { set_error("mdns_spectra_set_background: spectra are not in counts mode (mdns_spectra_set_counts comes first)"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_background: a joint state exists on these spectra (set the background first)"); return 1; }
	if (!bkg_counts) { set_error("mdns_spectra_set_background: null background counts"); return 1; }
	const int ndata = s->ndata, nx = s->nx;
	// the host copies are looked at before anything is uploaded; a pixel whose g is 0 or NaN or whose b is not finite is
	// masked: b = g = 0 here, and k_background_mask carries it to n and e
	const size_t n = (size_t) ndata * nx;
	std::vector<double> b_ok(n, 0.0), g_ok(n, 0.0);
	for (int k = 0; k < ndata; k++)
		for (int j = 0; j < nx; j++) {
			const size_t at = (size_t) k * nx + j;
			const double g = bkg_exposure ? bkg_exposure[at] : 1.0, b = bkg_counts[at];
			if (g < 0.0 || std::isinf(g)) {
				set_error("mdns_spectra_set_background: bkg_exposure[%d][%d] = %g: exposures must be finite and >= 0 (0 or NaN masks a pixel)", k, j, g);
				return 1;
			}
			if (b < 0.0 && !std::isinf(b) && g > 0.0) {
				set_error("mdns_spectra_set_background: bkg_counts[%d][%d] = %g: counts must be >= 0 (a non-finite one masks a pixel)", k, j, b);
				return 1;
			}
			if (g > 0.0 && std::isfinite(b)) { b_ok[at] = b; g_ok[at] = g; }
		}
	// made in locals and installed on success: the handle stays as it was when this call fails
	DeviceBuffer<double> d_b, d_g, d_kw;
	if (!device_rows(c, s, b_ok.data(), 0.0, d_b) || !device_rows(c, s, g_ok.data(), 0.0, d_g) || !device_offsets(c, s, offsets, d_kw)) return 1;
	if (ndata > 0 && nx > 0) {
		// a pixel masked on either side holds nothing on both (the slack and the channels past nx have e = 0 and g = 0 and
		// stay zero)
		const size_t elems = (size_t) ndata * s->ld + 2;
		hipLaunchKernelGGL(k_background_mask, dim3((unsigned) ((elems + 255) / 256)), dim3(256), 0, c->stream, s->d_y.get(), s->d_e.get(),
		                   d_b.get(), d_g.get(), elems);
		if (!launched("k_background_mask") || !spectra_changed(c, s)) return 1;
	}
	s->d_b = std::move(d_b);
	s->d_g = std::move(d_g);
	s->d_kw = std::move(d_kw);
	s->background = 1;
	return 0;
}
