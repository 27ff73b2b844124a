// Caller-defined models: the fixed-noise likelihood of sample.py:64-71 from model CURVES the caller made
// (include/mdns.h, mdns_curve_loglike_batch[_dev]) -- what K1 computes from (A, mu, sig), for any model.
//
//   L[b][k] = -0.5 sum_j ((curves[b][j] - y[row_k][j]) / noise)^2
//
// k_curve_rows   one workgroup = 128 selected spectra x 32 candidates.  Channels go by in stages of 32: the
//                stage's piece of the 128 spectrum rows (read from the [n_datasets x n_channels] rows, 256
//                contiguous bytes per row: a sparse selection costs exactly its own bytes) and of the 32 curves
//                are put into LDS, the next stage's loads already in flight in registers.  A lane owns TWO
//                spectra, a wave EIGHT candidates: 16 sums per lane in registers, so a spectrum value is read
//                from LDS once per eight candidates and a curve value -- the same address in all lanes, a
//                broadcast -- once per two spectra.  Per pair of channels a wave issues 10 16-byte LDS reads
//                (40 LDS cycles) against 64 fp64 instructions (256 cycles of its SIMD): with four SIMDs on one
//                LDS the arithmetic is what bounds it.
//
// Per (curve, spectrum) pair the sum is ONE chain: channels in ascending order, d = c - y, acc = fma(d, d, acc),
// from acc = 0; channels past the last one contribute fma(0, 0, acc), which changes nothing.  The value of a pair
// therefore does not depend on B, M, where either sits in its batch, or which entry point asked.  Nothing is
// validated: a non-finite curve value propagates as IEEE.
//
// The same curves at FIXED scale against per-pixel variances (include/mdns.h Part 9, mdns_curve_chi2_batch[_dev]):
//
//   L[b][k] = -0.5 sum_j w[row_k][j] (curves[b][j] - y[row_k][j])^2,   w = 1/v (s->d_w), w = 0 for a masked pixel
//
// k_curve_rows_w k_curve_rows' tiling with the weights staged exactly like the spectra: `ws` beside `ys`, both
//                [channel pair][spectrum] in 16-byte slots, 129 slots per channel pair.  Two separate arrays and not
//                {y, w} of one channel in one slot: a store group of ds_write_b128 is eight contiguous lanes -- eight
//                channel pairs of one spectrum --, and its banks are (address / 4) mod 32.  Here the eight lanes are
//                129 slots = 516 dwords apart, 4 mod 32: eight times four different banks, no conflict.  Interleaved,
//                a lane's two slots would be channels 2 cp and 2 cp + 1, the lanes 2 x 516 dwords = 8 mod 32 apart:
//                lanes cp and cp + 4 on the same banks, every store two-way.  LDS: 2 x 16 x 129 x 16 B + 8 KB =
//                74 240 B, two workgroups per CU.  Per pair of channels a wave issues 4 + 8 16-byte LDS reads (48 LDS
//                cycles) against 96 fp64 instructions (384 cycles of its SIMD): the arithmetic still bounds it.
//
// Per (curve, spectrum) pair the sum is ONE chain: channels in ascending order, from acc = +0:
//     d = c - y;  t = w * d (a rounded product);  acc = fma(t, d, acc);        L = -0.5 * acc
// Channels past the last one are staged as y = w = c = 0: fma(0 * 0, 0, acc) = acc.  A masked pixel -- w = 0 and a
// finite y (like.WeightedSpectra sees to both) -- gives t = +-0 and fma(+-0, d, acc) = acc for every finite d, bit for
// bit (acc = +0 stays +0: +0 + -0 = +0): the kernel does not look for masks.  As above, the bits of a pair do not
// depend on B, M, where either sits in its batch, ldc, the grid split or the entry point.
//
// The same curves as expected count RATES against photon counts (include/mdns.h Part 10, mdns_curve_poisson_batch[_dev]):
//
//   L[b][k] = sum_j ( n[row_k][j] log(max(c[b][j], tiny)) - e[row_k][j] c[b][j] ) + K[row_k],   tiny = DBL_MIN
//
// n = s->d_y (counts), e = s->d_e (exposures), K = s->d_koff (the host's sum n (1 + log e - log n)): -C/2 of the C
// statistic.  Two kernels:
//
// k_curve_log    curves [B][ldc] -> pairs {lc, c'} [B][ldp] (ldp = nx rounded up to a whole stage): c' = c for c >= 0
//                (-0 included) and NaN otherwise, lc = log(fmax(c', tiny)) by the device library's fp64 log; {0, 0}
//                behind channel nx.  One log per candidate and channel, never one per pair.
// k_curve_rows_p k_curve_rows_w's tiling -- 128 selected spectra x 32 candidates per workgroup, two spectra per lane,
//                eight candidates per wave, the next stage's loads in flight in registers -- in stages of SIXTEEN
//                channels.  Sixteen lanes still read one row per stage: lanes 0-7 its eight channel pairs of n, lanes
//                8-15 the same of e (2 x 128 contiguous bytes), into two [channel pair][spectrum] arrays of 16-byte
//                slots, 129 slots per pair.  The bank argument above holds unchanged: a store group of ds_write_b128 is
//                eight contiguous lanes -- the eight channel pairs of one spectrum in ONE of the two arrays --, 129
//                slots = 516 dwords = 4 mod 32 apart: eight times four different banks.  The curve stage holds the
//                pair {lc, c'} of a candidate and channel in one 16-byte slot, [candidate][channel]: a store group is
//                128 contiguous bytes, a read the same address in all lanes.  LDS: 2 x 8 x 129 x 16 B + 32 x 16 x 16 B
//                = 41 216 B, THREE workgroups per CU (123 648 of 163 840 B); registers allow the third (DESIGN section 4:
//                the figures).  Per pair of channels a wave issues 4 + 16 16-byte LDS reads (80 LDS cycles) against 64
//                fp64 instructions (256 cycles of its SIMD): with four SIMDs on one LDS, 320 cycles of LDS stand
//                against 256 of arithmetic -- the curve broadcast, twice k_curve_rows_w's, is what bounds this kernel,
//                still below that kernel's 384 cycles of arithmetic.
//
// Per (curve, spectrum) pair the sum is ONE chain: channels in ascending order, from acc = +0:
//     acc = fma(n, lc, acc);  acc = fma(-e, c', acc);                          L = acc + K
// Channels past the last one are staged as n = e = 0 and {lc, c'} = {0, 0}: fma(+-0, 0, acc) = acc.  A masked pixel
// is n = e = 0 (mdns_spectra_set_counts zeroes n where e = 0): fma(0, lc, acc) = acc and fma(-0, c', acc) = acc for
// every finite lc and c', bit for bit -- a deleted channel; the kernel does not look for masks.  c = +-0 gives
// lc = log(tiny), about -708.4: nothing where n = 0, n log(tiny) where n > 0, finite and ordered.  A negative or NaN
// curve value is c' = NaN, and fma(-e, NaN, acc) is NaN even at e = 0: NaN for every spectrum, which the accept test
// rejects.  +inf is not validated.  The bits of a pair do not depend on B, M, where either sits in its batch, ldc,
// the grid split or the entry point.
//
// Counts WITH A BACKGROUND spectrum per source spectrum (include/mdns.h Part 11, mdns_curve_wstat_batch[_dev]): the W
// statistic.  n, e as above; b = s->d_b the background region's counts, g = s->d_g its exposures (area ratio
// included); Kw = s->d_kw the host's offsets.  The background rate f of a pixel is unknown and profiled out of the joint
// Poisson likelihood of the two spectra, in closed form, per (candidate, spectrum, channel):
//
//   per pixel      T = e + g;  N = n + b;  Q = 4 (T b);  T2 = 2 T, or 1 where T == 0;  b2 = 2 b
//   wstat_rate     a = fma(-T, c', N);  d = sqrt(fma(a, a, Q c'));
//                  f = (a + d) / T2 where a >= 0,  f = (b2 c') / (d - a) where not        (the branch that does not cancel)
//   wstat_term     s = c' + f
//                  acc = fma(n, log(fmax(s, tiny)), acc);  acc = fma(b, log(fmax(f, tiny)), acc);
//                  acc = fma(-e, s, acc);                  acc = fma(-g, f, acc)
//   L[b][k] = acc + Kw[row_k], the chain over the channels in ascending order from acc = +0
//
// with the device library's fp64 log, sqrt and division; c' = c for c >= 0 (-0 included) and NaN otherwise, made in the
// fetch (no pre-pass: nothing can be staged per candidate, f depends on all three indices).  The per-pixel values are
// made in registers from the four staged ones, once per lane, channel and stage: nothing derived is kept in memory.
//
// k_curve_rows_b  64 selected spectra x 4 candidates per workgroup: one spectrum per lane, one candidate per wave, ONE
//                chain per lane.  A pair and channel costs about 150 fp64 instructions (two inlined logarithms, a
//                square root, a division: DESIGN section 4 has the count), so neither LDS nor loads bound the kernel
//                and the tile is as small as the staging allows -- the small tile spreads a chunk of a few thousand
//                pairs over the chip, which is what shortens it.  Stages of sixteen channels as in k_curve_rows_p:
//                32 lanes read one row per stage, eight channel pairs of each of n, e, b, g (4 x 128 contiguous bytes),
//                into four [channel pair][spectrum] arrays of 16-byte slots, 65 slots per pair (260 dwords = 4 mod 32
//                apart: the eight lanes of a ds_write_b128 store group fall on eight times four different banks).
//                The curve stage is [candidate][channel], filled by the first wave.  LDS 4 x 8 x 65 x 16 B + 4 x 16 x
//                8 B = 33 792 B.  The next stage's loads are in flight in registers.
// k_curve_background  the same wstat_pixel and wstat_rate, elementwise: f [B][M][nx] (mdns_curve_background_batch).
//
// A masked pixel is n = e = b = g = 0 (mdns_spectra_set_background zeroes all four where any side is masked), and a
// channel past the last one is staged the same with c' = 0: T = N = Q = b2 = 0 and T2 = 1, so a = fma(-0, c', 0) = +0,
// d = sqrt(0) = 0, f = (0 + 0) / 1 = 0 -- no 0/0 --, s = c' + 0 = c', and the four fma add +-0 to acc for every finite
// c' >= 0 (log(fmax(., tiny)) is finite): a deleted channel, bit for bit.  The guard is T2, a per-pixel value; no
// candidate is tested.  A NaN c' makes a, d, f, s NaN; fmax drops it from the logarithms, fma(-e, NaN, acc) is NaN
// even at e = 0: NaN for every spectrum of that candidate.  c' = +-0 with n > 0, b = 0: a = N, f = 2 N / (2 T) = n / T.
#include "mdns_internal.h"

#include <cfloat>
#include <cmath>
#include <vector>

namespace mdns {

static constexpr int kCurveSpectra = 128;                 // spectra per workgroup (two per lane)
static constexpr int kCurveNC = 8;                        // candidates per wave, all in registers
static constexpr int kCurveCands = 4 * kCurveNC;          // candidates per workgroup
static constexpr int kCurveCH = 32;                       // channels per stage
// 16-byte slots per channel pair in LDS: one more than the spectra, so that the eight lanes of a store group --
// eight channel pairs of one spectrum -- fall on eight different groups of four banks
static constexpr int kCurveSlots = kCurveSpectra + 1;

__global__ __launch_bounds__(256) void k_curve_rows(
    const double *__restrict__ Y, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double scale, double *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) double2 ys[kCurveCH / 2][kCurveSlots];       // [channel pair][spectrum]
	__shared__ __attribute__((aligned(16))) double cs[kCurveCands][kCurveCH];            // [candidate][channel]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int k0 = blockIdx.x * kCurveSpectra, b0 = blockIdx.y * kCurveCands;
	// what this thread brings in per stage: channel pair cp of the spectra rsub, rsub + 16, ... (sixteen lanes
	// read the 256 bytes of one row), and channel cch of the candidates crow, crow + 8, ...
	const int cp = lane & 15, rsub = wave * 4 + (lane >> 4);
	const int cch = threadIdx.x & 31, crow = threadIdx.x >> 5;
	const double *yrow[kCurveSpectra / 16];
#pragma unroll
	for (int i = 0; i < kCurveSpectra / 16; i++) {
		const int k = k0 + rsub + 16 * i;
		const int kk = k < M ? k : M - 1;                                     // (past the selection: its last row again, never stored)
		yrow[i] = Y + (size_t) (rows ? rows[kk] : kk) * ld + 2 * cp;
	}
	double2 yv[kCurveSpectra / 16];
	double cv[kCurveCands / 8];
	auto fetch = [&](int j0) {
		const int j = j0 + 2 * cp;
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) {
			// (rows are 16-byte aligned and an even number of doubles long: the pair of an even channel below nx is inside)
			double2 v = make_double2(0.0, 0.0);
			if (j < nx) v = *reinterpret_cast<const double2 *>(yrow[i] + j0);
			if (j + 1 >= nx) v.y = 0.0;
			yv[i] = v;
		}
#pragma unroll
		for (int i = 0; i < kCurveCands / 8; i++) {
			const int b = b0 + crow + 8 * i;
			cv[i] = b < B && j0 + cch < nx ? curves[(size_t) b * ldc + j0 + cch] : 0.0;
		}
	};
	double acc[kCurveNC][2];
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) acc[c][0] = acc[c][1] = 0.0;
	const bool working = b0 + wave * kCurveNC < B;                            // wave-uniform; an idle wave still stages
	fetch(0);
	for (int j0 = 0; j0 < nx; j0 += kCurveCH) {
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) ys[cp][rsub + 16 * i] = yv[i];
#pragma unroll
		for (int i = 0; i < kCurveCands / 8; i++) cs[crow + 8 * i][cch] = cv[i];
		__syncthreads();
		if (j0 + kCurveCH < nx) fetch(j0 + kCurveCH);
		if (working) {
#pragma unroll 4
			for (int jp = 0; jp < kCurveCH / 2; jp++) {
				const double2 ya = ys[jp][lane], yb = ys[jp][lane + 64];
#pragma unroll
				for (int c = 0; c < kCurveNC; c++) {
					const double2 m = *reinterpret_cast<const double2 *>(&cs[wave * kCurveNC + c][2 * jp]);
					double d;
					d = m.x - ya.x; acc[c][0] = fma(d, d, acc[c][0]);
					d = m.y - ya.y; acc[c][0] = fma(d, d, acc[c][0]);
					d = m.x - yb.x; acc[c][1] = fma(d, d, acc[c][1]);
					d = m.y - yb.y; acc[c][1] = fma(d, d, acc[c][1]);
				}
			}
		}
		__syncthreads();
	}
	if (!working) return;
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) {
		const int b = b0 + wave * kCurveNC + c;
		if (b >= B) break;
		const int k = k0 + lane;
		if (k < M) out[(size_t) b * M + k] = acc[c][0] * scale;
		if (k + 64 < M) out[(size_t) b * M + k + 64] = acc[c][1] * scale;
	}
}

// The fixed-scale chi^2 with per-pixel weights W [ndata][ld] (the handle's 1 / v): k_curve_rows with `ws` staged
// beside `ys` (file header: layout, chain).  Spectrum pieces of Y and W come from the same row offsets.
__global__ __launch_bounds__(256) void k_curve_rows_w(
    const double *__restrict__ Y, const double *__restrict__ W, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) double2 ys[kCurveCH / 2][kCurveSlots];       // [channel pair][spectrum]
	__shared__ __attribute__((aligned(16))) double2 ws[kCurveCH / 2][kCurveSlots];       // the same of the weights
	__shared__ __attribute__((aligned(16))) double cs[kCurveCands][kCurveCH];            // [candidate][channel]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int k0 = blockIdx.x * kCurveSpectra, b0 = blockIdx.y * kCurveCands;
	const int cp = lane & 15, rsub = wave * 4 + (lane >> 4);
	const int cch = threadIdx.x & 31, crow = threadIdx.x >> 5;
	size_t at[kCurveSpectra / 16];                                            // of this thread's channel pair in its rows
#pragma unroll
	for (int i = 0; i < kCurveSpectra / 16; i++) {
		const int k = k0 + rsub + 16 * i;
		const int kk = k < M ? k : M - 1;                                     // (past the selection: its last row again, never stored)
		at[i] = (size_t) (rows ? rows[kk] : kk) * ld + 2 * cp;
	}
	double2 yv[kCurveSpectra / 16], wv[kCurveSpectra / 16];
	double cv[kCurveCands / 8];
	auto fetch = [&](int j0) {
		const int j = j0 + 2 * cp;
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) {
			// (rows are 16-byte aligned and an even number of doubles long: the pair of an even channel below nx is inside)
			double2 y = make_double2(0.0, 0.0), w = make_double2(0.0, 0.0);
			if (j < nx) {
				y = *reinterpret_cast<const double2 *>(Y + at[i] + j0);
				w = *reinterpret_cast<const double2 *>(W + at[i] + j0);
			}
			if (j + 1 >= nx) y.y = w.y = 0.0;
			yv[i] = y; wv[i] = w;
		}
#pragma unroll
		for (int i = 0; i < kCurveCands / 8; i++) {
			const int b = b0 + crow + 8 * i;
			cv[i] = b < B && j0 + cch < nx ? curves[(size_t) b * ldc + j0 + cch] : 0.0;
		}
	};
	double acc[kCurveNC][2];
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) acc[c][0] = acc[c][1] = 0.0;
	const bool working = b0 + wave * kCurveNC < B;                            // wave-uniform; an idle wave still stages
	fetch(0);
	for (int j0 = 0; j0 < nx; j0 += kCurveCH) {
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) { ys[cp][rsub + 16 * i] = yv[i]; ws[cp][rsub + 16 * i] = wv[i]; }
#pragma unroll
		for (int i = 0; i < kCurveCands / 8; i++) cs[crow + 8 * i][cch] = cv[i];
		__syncthreads();
		if (j0 + kCurveCH < nx) fetch(j0 + kCurveCH);
		if (working) {
#pragma unroll 4
			for (int jp = 0; jp < kCurveCH / 2; jp++) {
				const double2 ya = ys[jp][lane], yb = ys[jp][lane + 64];
				const double2 wa = ws[jp][lane], wb = ws[jp][lane + 64];
#pragma unroll
				for (int c = 0; c < kCurveNC; c++) {
					const double2 m = *reinterpret_cast<const double2 *>(&cs[wave * kCurveNC + c][2 * jp]);
					double d;
					d = m.x - ya.x; acc[c][0] = fma(__dmul_rn(wa.x, d), d, acc[c][0]);
					d = m.y - ya.y; acc[c][0] = fma(__dmul_rn(wa.y, d), d, acc[c][0]);
					d = m.x - yb.x; acc[c][1] = fma(__dmul_rn(wb.x, d), d, acc[c][1]);
					d = m.y - yb.y; acc[c][1] = fma(__dmul_rn(wb.y, d), d, acc[c][1]);
				}
			}
		}
		__syncthreads();
	}
	if (!working) return;
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) {
		const int b = b0 + wave * kCurveNC + c;
		if (b >= B) break;
		const int k = k0 + lane;
		if (k < M) out[(size_t) b * M + k] = -0.5 * acc[c][0];
		if (k + 64 < M) out[(size_t) b * M + k + 64] = -0.5 * acc[c][1];
	}
}

// ---- counts: the Poisson likelihood (file header) ----
static constexpr int kCountCH = 16;                       // channels per stage of k_curve_rows_p
// row stride, in {lc, c'} pairs, of the block k_curve_log stages: whole stages, so that k_curve_rows_p tests no channel
static inline int count_ld(int nx) { return (nx + kCountCH - 1) / kCountCH * kCountCH; }

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

// L[b][k] = sum_j (n lc - e c') + K from the staged pairs P [B][ldp] (k_curve_log), the counts Y and exposures E
// [ndata][ld] and the offsets K [ndata]: k_curve_rows_w's tiling in stages of sixteen channels (file header: layout, chain)
__global__ __launch_bounds__(256) void k_curve_rows_p(
    const double *__restrict__ Y, const double *__restrict__ E, const double *__restrict__ K, int ld, int nx,
    const double2 *__restrict__ P, int ldp, int B, const int *__restrict__ rows, int M, double *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) double2 ne[2][kCountCH / 2][kCurveSlots];    // n, e: [channel pair][spectrum]
	__shared__ __attribute__((aligned(16))) double2 ps[kCurveCands][kCountCH];           // {lc, c'}: [candidate][channel]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int k0 = blockIdx.x * kCurveSpectra, b0 = blockIdx.y * kCurveCands;
	// what this thread brings in per stage: channel pair cp of n (lanes 0-7 of sixteen) or of e (lanes 8-15) of the
	// spectra rsub, rsub + 16, ... (sixteen lanes read 2 x 128 bytes of one row), and channel cch of the candidates
	// crow, crow + 16
	const int cp = lane & 7, which = (lane >> 3) & 1, rsub = wave * 4 + (lane >> 4);
	const int cch = threadIdx.x & 15, crow = threadIdx.x >> 4;
	const double *src[kCurveSpectra / 16];
#pragma unroll
	for (int i = 0; i < kCurveSpectra / 16; i++) {
		const int k = k0 + rsub + 16 * i;
		const int kk = k < M ? k : M - 1;                                     // (past the selection: its last row again, never stored)
		src[i] = (which ? E : Y) + (size_t) (rows ? rows[kk] : kk) * ld + 2 * cp;
	}
	double2 sv[kCurveSpectra / 16], pv[kCurveCands / 16];
	auto fetch = [&](int j0) {
		const int j = j0 + 2 * cp;
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) {
			// (rows are 16-byte aligned and an even number of doubles long: the pair of an even channel below nx is inside)
			double2 v = make_double2(0.0, 0.0);
			if (j < nx) v = *reinterpret_cast<const double2 *>(src[i] + j0);
			if (j + 1 >= nx) v.y = 0.0;
			sv[i] = v;
		}
#pragma unroll
		for (int i = 0; i < kCurveCands / 16; i++) {
			const int b = b0 + crow + 16 * i;
			pv[i] = b < B ? P[(size_t) b * ldp + j0 + cch] : make_double2(0.0, 0.0);          // (j0 + cch < ldp: whole stages)
		}
	};
	double acc[kCurveNC][2];
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) acc[c][0] = acc[c][1] = 0.0;
	const bool working = b0 + wave * kCurveNC < B;                            // wave-uniform; an idle wave still stages
	fetch(0);
	for (int j0 = 0; j0 < nx; j0 += kCountCH) {
#pragma unroll
		for (int i = 0; i < kCurveSpectra / 16; i++) ne[which][cp][rsub + 16 * i] = sv[i];
#pragma unroll
		for (int i = 0; i < kCurveCands / 16; i++) ps[crow + 16 * i][cch] = pv[i];
		__syncthreads();
		if (j0 + kCountCH < nx) fetch(j0 + kCountCH);
		if (working) {
#pragma unroll 4
			for (int jp = 0; jp < kCountCH / 2; jp++) {
				const double2 na = ne[0][jp][lane], nb = ne[0][jp][lane + 64];
				const double2 ea = ne[1][jp][lane], eb = ne[1][jp][lane + 64];
#pragma unroll
				for (int c = 0; c < kCurveNC; c++) {
					const double2 p = ps[wave * kCurveNC + c][2 * jp], q = ps[wave * kCurveNC + c][2 * jp + 1];
					acc[c][0] = fma(na.x, p.x, acc[c][0]); acc[c][0] = fma(-ea.x, p.y, acc[c][0]);
					acc[c][0] = fma(na.y, q.x, acc[c][0]); acc[c][0] = fma(-ea.y, q.y, acc[c][0]);
					acc[c][1] = fma(nb.x, p.x, acc[c][1]); acc[c][1] = fma(-eb.x, p.y, acc[c][1]);
					acc[c][1] = fma(nb.y, q.x, acc[c][1]); acc[c][1] = fma(-eb.y, q.y, acc[c][1]);
				}
			}
		}
		__syncthreads();
	}
	if (!working) return;
	const int ka = k0 + lane, kb = ka + 64;
	const double Ka = ka < M ? K[rows ? rows[ka] : ka] : 0.0, Kb = kb < M ? K[rows ? rows[kb] : kb] : 0.0;
#pragma unroll
	for (int c = 0; c < kCurveNC; c++) {
		const int b = b0 + wave * kCurveNC + c;
		if (b >= B) break;
		if (ka < M) out[(size_t) b * M + ka] = acc[c][0] + Ka;
		if (kb < M) out[(size_t) b * M + kb] = acc[c][1] + Kb;
	}
}

// y[i] = 0 where e[i] == 0, over the whole [ndata][ld] block (mdns_spectra_set_counts: a masked pixel holds no counts)
__global__ __launch_bounds__(256) void k_counts_mask(double *__restrict__ y, const double *__restrict__ e, size_t n)
{
	const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
	if (i < n && e[i] == 0.0) y[i] = 0.0;
}

// ---- counts with a background: the W statistic (file header) ----
static constexpr int kBgSpectra = 64;                     // spectra per workgroup of k_curve_rows_b (one per lane)
static constexpr int kBgCands = 4;                        // candidates per workgroup (one per wave)
static constexpr int kBgCH = 16;                          // channels per stage
static constexpr int kBgSlots = kBgSpectra + 1;           // 16-byte slots per channel pair (file header: banks)

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

// L[b][k] = sum_j wstat_term + Kw from the counts Y, exposures E, background counts Bc and exposures G [ndata][ld],
// the offsets Kw [ndata] and the curves [B][ldc] (file header: tile, staging, chain)
__global__ __launch_bounds__(256) void k_curve_rows_b(
    const double *__restrict__ Y, const double *__restrict__ E, const double *__restrict__ Bc, const double *__restrict__ G,
    const double *__restrict__ Kw, int ld, int nx, const double *__restrict__ curves, int ldc, int B,
    const int *__restrict__ rows, int M, double *__restrict__ out)
{
	__shared__ __attribute__((aligned(16))) double2 px[4][kBgCH / 2][kBgSlots];          // n, e, b, g: [channel pair][spectrum]
	__shared__ __attribute__((aligned(16))) double cs[kBgCands][kBgCH];                  // c': [candidate][channel]
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int k0 = blockIdx.x * kBgSpectra, b0 = blockIdx.y * kBgCands;
	// what this thread brings in per stage: channel pair cp of array `which` of the spectra rsub, rsub + 8, ... (32 lanes
	// read 4 x 128 bytes of one row); the first wave also channel cch of candidate crow
	const int cp = threadIdx.x & 7, which = (threadIdx.x >> 3) & 3, rsub = threadIdx.x >> 5;
	const int cch = threadIdx.x & 15, crow = threadIdx.x >> 4;
	const double *const base = which == 0 ? Y : which == 1 ? E : which == 2 ? Bc : G;
	const double *src[kBgSpectra / 8];
#pragma unroll
	for (int i = 0; i < kBgSpectra / 8; i++) {
		const int k = k0 + rsub + 8 * i;
		const int kk = k < M ? k : M - 1;                                     // (past the selection: its last row again, never stored)
		src[i] = base + (size_t) (rows ? rows[kk] : kk) * ld + 2 * cp;
	}
	const bool curve_lane = crow < kBgCands;                                  // (the first wave)
	const double *csrc = nullptr;
	if (curve_lane && b0 + crow < B) csrc = curves + (size_t) (b0 + crow) * ldc + cch;
	double2 sv[kBgSpectra / 8];
	double cv = 0.0;
	auto fetch = [&](int j0) {
		const int j = j0 + 2 * cp;
#pragma unroll
		for (int i = 0; i < kBgSpectra / 8; i++) {
			// (rows are 16-byte aligned and an even number of doubles long: the pair of an even channel below nx is inside)
			double2 v = make_double2(0.0, 0.0);
			if (j < nx) v = *reinterpret_cast<const double2 *>(src[i] + j0);
			if (j + 1 >= nx) v.y = 0.0;
			sv[i] = v;
		}
		cv = 0.0;
		if (csrc && j0 + cch < nx) {
			const double c = csrc[j0];
			cv = c >= 0.0 ? c : (double) NAN;
		}
	};
	double acc = 0.0;
	const bool working = b0 + wave < B;                                       // wave-uniform; an idle wave still stages
	fetch(0);
	for (int j0 = 0; j0 < nx; j0 += kBgCH) {
#pragma unroll
		for (int i = 0; i < kBgSpectra / 8; i++) px[which][cp][rsub + 8 * i] = sv[i];
		if (curve_lane) cs[crow][cch] = cv;
		__syncthreads();
		if (j0 + kBgCH < nx) fetch(j0 + kBgCH);
		if (working) {
#pragma unroll 1
			for (int jp = 0; jp < kBgCH / 2; jp++) {
				const double2 n2 = px[0][jp][lane], e2 = px[1][jp][lane], b2 = px[2][jp][lane], g2 = px[3][jp][lane];
				const double c0 = cs[wave][2 * jp], c1 = cs[wave][2 * jp + 1];
				acc = wstat_term(wstat_pixel(n2.x, e2.x, b2.x, g2.x), c0, acc);
				acc = wstat_term(wstat_pixel(n2.y, e2.y, b2.y, g2.y), c1, acc);
			}
		}
		__syncthreads();
	}
	if (!working) return;
	const int k = k0 + lane;
	if (k < M) out[(size_t) (b0 + wave) * M + k] = acc + Kw[rows ? rows[k] : k];
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

bool launch_curve_rows(const mdns_spectra *s, const double *d_curves, int ldc, int B, double scale,
                       const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0) return true;
	const dim3 grid((M + kCurveSpectra - 1) / kCurveSpectra, (B + kCurveCands - 1) / kCurveCands);
	hipLaunchKernelGGL(k_curve_rows, grid, dim3(256), 0, c->stream, (const double *) s->d_y.get(), s->ld, s->nx, d_curves, ldc, B,
	                   d_rows, M, scale, d_out);
	return launched("k_curve_rows");
}

bool launch_curve_rows_w(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0) return true;
	const dim3 grid((M + kCurveSpectra - 1) / kCurveSpectra, (B + kCurveCands - 1) / kCurveCands);
	hipLaunchKernelGGL(k_curve_rows_w, grid, dim3(256), 0, c->stream, (const double *) s->d_y.get(), (const double *) s->d_w.get(), s->ld, s->nx,
	                   d_curves, ldc, B, d_rows, M, d_out);
	return launched("k_curve_rows_w");
}

bool launch_curve_poisson(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0) return true;
	const int ldp = count_ld(s->nx);
	if (!ensure_model(s, (size_t) B * ldp * 2)) return false;
	double2 *staged = reinterpret_cast<double2 *>(s->d_model.get());
	hipLaunchKernelGGL(k_curve_log, dim3((ldp + 255) / 256, B), dim3(256), 0, c->stream, d_curves, ldc, s->nx, staged, ldp);
	if (!launched("k_curve_log")) return false;
	const dim3 grid((M + kCurveSpectra - 1) / kCurveSpectra, (B + kCurveCands - 1) / kCurveCands);
	hipLaunchKernelGGL(k_curve_rows_p, grid, dim3(256), 0, c->stream, (const double *) s->d_y.get(), (const double *) s->d_e.get(),
	                   (const double *) s->d_koff.get(), s->ld, s->nx, (const double2 *) staged, ldp, B, d_rows, M, d_out);
	return launched("k_curve_rows_p");
}

bool launch_curve_wstat(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_rows, int M, double *d_out)
{
	Context *c = ctx();
	if (B <= 0 || M <= 0) return true;
	const dim3 grid((M + kBgSpectra - 1) / kBgSpectra, (B + kBgCands - 1) / kBgCands);
	hipLaunchKernelGGL(k_curve_rows_b, grid, dim3(256), 0, c->stream, (const double *) s->d_y.get(), (const double *) s->d_e.get(),
	                   (const double *) s->d_b.get(), (const double *) s->d_g.get(), (const double *) s->d_kw.get(), s->ld, s->nx,
	                   d_curves, ldc, B, d_rows, M, d_out);
	return launched("k_curve_rows_b");
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

// what the device entry points check first; 1: refused, 0: go on, -1: nothing to score.  needs: what the likelihood asks
// of the handle
enum { kNeedsNothing = 0, kNeedsVariances = 1, kNeedsCounts = 2, kNeedsBackground = 3 };
static int curve_batch_check(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                             const double *d_Lout, int needs, const char *who)
{
	if (!ctx()) return 1;
	if (!s) { set_error("%s: null spectra handle", who); return 1; }
	if (B < 0 || M < 0 || M > s->ndata || s->nx < 1 || ldc < s->nx || (!d_row_ids && M != s->ndata && M != 0)) {
		set_error("%s: bad sizes B=%d M=%d (ndata=%d) ldc=%d (nx=%d)", who, B, M, s->ndata, ldc, s->nx);
		return 1;
	}
	if (needs == kNeedsVariances && !s->d_w.get()) { set_error("%s: spectra were created without variances", who); return 1; }
	if (needs == kNeedsCounts && !s->counts) { set_error("%s: spectra are not in counts mode (mdns_spectra_set_counts)", who); return 1; }
	if (needs == kNeedsBackground && !s->background) { set_error("%s: spectra have no background (mdns_spectra_set_background)", who); return 1; }
	if (B == 0 || M == 0) return -1;
	if (!d_curves || !d_Lout) { set_error("%s: null argument", who); return 1; }
	return 0;
}

extern "C" int mdns_curve_loglike_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                                            const int *d_row_ids, int M, double *d_Lout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_Lout, kNeedsNothing, "mdns_curve_loglike_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_curve_rows(s, d_curves, ldc, B, -0.5 / (noise_level * noise_level), d_row_ids, M, d_Lout) ? 0 : 1;
}

extern "C" int mdns_curve_chi2_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                         double *d_Lout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_Lout, kNeedsVariances, "mdns_curve_chi2_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_curve_rows_w(s, d_curves, ldc, B, d_row_ids, M, d_Lout) ? 0 : 1;
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

extern "C" int mdns_curve_poisson_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                            double *d_Lout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_Lout, kNeedsCounts, "mdns_curve_poisson_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_curve_poisson(s, d_curves, ldc, B, d_row_ids, M, d_Lout) ? 0 : 1;
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
	const int ndata = s->ndata, nx = s->nx, ld = s->ld;
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
	// rows as the kernels read them: [ndata][ld] with the slack of d_y, zero behind channel nx
	const size_t elems = (size_t) ndata * ld + 2;
	std::vector<double> e_rows(elems, 0.0), koff((size_t) (ndata > 0 ? ndata : 1), 0.0);
	for (int k = 0; k < ndata; k++)
		for (int j = 0; j < nx; j++) e_rows[(size_t) k * ld + j] = exposure ? exposure[(size_t) k * nx + j] : 1.0;
	if (offsets) for (int k = 0; k < ndata; k++) koff[k] = offsets[k];
	// made in locals and installed on success: the handle stays as it was when this call fails
	DeviceBuffer<double> d_e, d_koff;
	if (!d_e.make(elems) || !d_koff.make(koff.size())) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(d_e.get(), e_rows.data(), elems * sizeof(double), hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipMemcpyAsync(d_koff.get(), koff.data(), koff.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
	if (any_zero && ndata > 0 && nx > 0) {
		// a masked pixel holds no counts; what the handle keeps derived from y follows (the Gaussian batch functions then
		// score the y that is on the handle)
		hipLaunchKernelGGL(k_counts_mask, dim3((unsigned) ((elems + 255) / 256)), dim3(256), 0, c->stream, s->d_y.get(), (const double *) d_e.get(), elems);
		if (!launched("k_counts_mask")) return 1;
		bool ok = true;
		if (s->d_yT.get()) ok = launch_tile_columns(s->d_y.get(), ld, ndata, nx, nullptr, s->d_yT.get());
		if (ok && s->d_ysq.get()) ok = launch_row_sumsq(s->d_y.get(), ld, nx, ndata, s->d_ysq.get());
		if (!ok || !MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
		s->d_yG.release();                                        // (made again from the new y on first use)
	}
	s->d_e = std::move(d_e);
	s->d_koff = std::move(d_koff);
	s->counts = 1;
	return 0;
}

// ---- counts with a background (mdns.h Part 11) ----
extern "C" int mdns_curve_wstat_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                          double *d_Lout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_Lout, kNeedsBackground, "mdns_curve_wstat_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_curve_wstat(s, d_curves, ldc, B, d_row_ids, M, d_Lout) ? 0 : 1;
}

extern "C" int mdns_curve_background_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                               double *d_fout)
{
	const int rc = curve_batch_check(s, d_curves, ldc, B, d_row_ids, M, d_fout, kNeedsBackground, "mdns_curve_background_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_curve_background(s, d_curves, ldc, B, d_row_ids, M, d_fout) ? 0 : 1;
}

extern "C" int mdns_curve_background_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *fout)
{
	Context *c = ctx();
	const int rc = curve_batch_check(s, curves, s ? s->nx : 0, B, row_ids, M, fout, kNeedsBackground, "mdns_curve_background_batch");
	if (rc != 0) return rc > 0;
	if (row_ids) {
		for (int k = 0; k < M; k++)
			if (row_ids[k] < 0 || row_ids[k] >= s->ndata) {
				set_error("mdns_curve_background_batch: row_ids[%d]=%d outside [0,%d)", k, row_ids[k], s->ndata);
				return 1;
			}
	}
	const size_t np = (size_t) B * s->nx, no = (size_t) B * M * s->nx;
	if (!s->d_params.fit(np) || !s->d_out.fit(no) || (row_ids && !s->d_rows.fit((size_t) M))) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(s->d_params.get(), curves, np * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (row_ids && !MDNS_HIP(hipMemcpyAsync(s->d_rows.get(), row_ids, (size_t) M * sizeof(int), hipMemcpyHostToDevice, c->stream))) return 1;
	if (!launch_curve_background(s, s->d_params.get(), s->nx, B, row_ids ? s->d_rows.get() : nullptr, M, s->d_out.get())) return 1;
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
	const int ndata = s->ndata, nx = s->nx, ld = s->ld;
	// the host copies are looked at before anything is uploaded
	for (int k = 0; k < ndata; k++)
		for (int j = 0; j < nx; j++) {
			const double g = bkg_exposure ? bkg_exposure[(size_t) k * nx + j] : 1.0, b = bkg_counts[(size_t) k * nx + j];
			if (g < 0.0 || std::isinf(g)) {
				set_error("mdns_spectra_set_background: bkg_exposure[%d][%d] = %g: exposures must be finite and >= 0 (0 or NaN masks a pixel)", k, j, g);
				return 1;
			}
			if (b < 0.0 && !std::isinf(b) && g > 0.0) {
				set_error("mdns_spectra_set_background: bkg_counts[%d][%d] = %g: counts must be >= 0 (a non-finite one masks a pixel)", k, j, b);
				return 1;
			}
		}
	// rows as the kernels read them: [ndata][ld] with the slack of d_y, zero behind channel nx; a pixel whose g is 0 or
	// NaN or whose b is not finite is masked: b = g = 0 here, and k_background_mask carries it to n and e
	const size_t elems = (size_t) ndata * ld + 2;
	std::vector<double> b_rows(elems, 0.0), g_rows(elems, 0.0), kw((size_t) (ndata > 0 ? ndata : 1), 0.0);
	for (int k = 0; k < ndata; k++)
		for (int j = 0; j < nx; j++) {
			const double g = bkg_exposure ? bkg_exposure[(size_t) k * nx + j] : 1.0, b = bkg_counts[(size_t) k * nx + j];
			if (!(g > 0.0) || !std::isfinite(b)) continue;
			b_rows[(size_t) k * ld + j] = b;
			g_rows[(size_t) k * ld + j] = g;
		}
	if (offsets) for (int k = 0; k < ndata; k++) kw[k] = offsets[k];
	// made in locals and installed on success: the handle stays as it was when this call fails
	DeviceBuffer<double> d_b, d_g, d_kw;
	if (!d_b.make(elems) || !d_g.make(elems) || !d_kw.make(kw.size())) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(d_b.get(), b_rows.data(), elems * sizeof(double), hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipMemcpyAsync(d_g.get(), g_rows.data(), elems * sizeof(double), hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipMemcpyAsync(d_kw.get(), kw.data(), kw.size() * sizeof(double), hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
	if (ndata > 0 && nx > 0) {
		// a pixel masked on either side holds nothing on both; what the handle keeps derived from y follows, as in
		// mdns_spectra_set_counts (the slack and the channels past nx have e = 0 and g = 0 and stay zero)
		hipLaunchKernelGGL(k_background_mask, dim3((unsigned) ((elems + 255) / 256)), dim3(256), 0, c->stream, s->d_y.get(), s->d_e.get(),
		                   d_b.get(), d_g.get(), elems);
		if (!launched("k_background_mask")) return 1;
		bool ok = true;
		if (s->d_yT.get()) ok = launch_tile_columns(s->d_y.get(), ld, ndata, nx, nullptr, s->d_yT.get());
		if (ok && s->d_ysq.get()) ok = launch_row_sumsq(s->d_y.get(), ld, nx, ndata, s->d_ysq.get());
		if (!ok || !MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
		s->d_yG.release();                                        // (made again from the new y on first use)
	}
	s->d_b = std::move(d_b);
	s->d_g = std::move(d_g);
	s->d_kw = std::move(d_kw);
	s->background = 1;
	return 0;
}
