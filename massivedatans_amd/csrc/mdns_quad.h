// The quad-lane scorer of a draw chunk, in the pieces its kernels are made of (k_chunk_accept and k_exact_list in
// mdns_chunk.hip, k_chain_accept in mdns_chain.hip).
//
// Work of one workgroup (256 threads): 64 selected spectra (one tile of the selection) x 4 candidates.  A quad of lanes
// shares ONE spectrum: lane q of the quad LOADS the q-th quarter of every 64-byte stage of the row (so four adjacent
// lanes read one cache line and a wave's load touches 16 lines -- with one lane per spectrum it would be 64 lines four
// times over, and the texture-address unit, one line per clock, was the bound: 33 us measured), and SCORES candidate q
// of the four against the whole spectrum, the other three quarters of a stage arriving by quad broadcasts (DPP moves
// inside the VALU).  The chain of a (candidate, spectrum) pair is that of every other K1 form: one accumulator,
// channels ascending, d = m - y, acc = fma(d, d, acc), padding channels contributing fma(0, 0, acc) -- so a likelihood
// does not depend on which kernel computed it.
#pragma once
#include "mdns_internal.h"

#ifdef __HIPCC__
namespace mdns {

static constexpr int kCH = 8;              // channels per stage

// quad broadcast: every lane of a quad gets the value lane Q of the quad holds (DPP quad_perm)
template <int Q>
__device__ __forceinline__ double quad_bcast(double v)
{
	constexpr int ctrl = Q | (Q << 2) | (Q << 4) | (Q << 6);
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), ctrl, 0xf, 0xf, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), ctrl, 0xf, 0xf, true);
	return __hiloint2double(hi, lo);
}

// This quad's spectrum: quarter q of every stage of row `row` into y, the whole row requested before the first sum
// starts (NST = stages held in registers); channels at or beyond the row's length are padding: zeros.  Returns the
// threshold the spectrum's data set has to beat.
template <int NST>
__device__ __forceinline__ double quad_load_row(const double *__restrict__ Y, int ld, int row, bool live, int q,
                                                const double *__restrict__ higher, double2 (&y)[NST])
{
	const double *yr = Y + (size_t) row * ld;
#pragma unroll
	for (int s = 0; s < NST; s++) {
		const int j = s * kCH + 2 * q;
		const double2 v = *reinterpret_cast<const double2 *>(yr + (j < ld ? j : 0));
		y[s].x = j < ld ? v.x : 0.0;
		y[s].y = j < ld ? v.y : 0.0;
	}
	return live ? higher[row] : __builtin_nan("");                     // NaN compares false: no vote
}

// Templates of candidates first .. first + 3 from their parameters par [4][3] (LDS), computed here (clike.c:65:
// A exp(-0.5 ((mu - x)/sig)^2)), into tpl [nxp / 2][4 candidates] pairs of channels; zero for candidates at or beyond
// B and for padding channels
__device__ __forceinline__ void quad_templates(double *__restrict__ tpl, const double *__restrict__ par,
                                               const double *__restrict__ xgrid, int nx, int nxp, int first, int B)
{
	for (int e = threadIdx.x; e < nxp * 4; e += 256) {
		const int j = e >> 2, bb = e & 3;
		double m = 0.0;
		if (j < nx && first + bb < B) {
			const double A = par[bb * 3], mu = par[bb * 3 + 1], sig = par[bb * 3 + 2];
			const double t = (mu - xgrid[j]) / sig;
			m = A * exp(-0.5 * (t * t));
		}
		tpl[((size_t) (j >> 1) * 4 + bb) * 2 + (j & 1)] = m;
	}
}

// The same layout filled with the columns of the listed candidates list[g .. g + 3] (zero at or beyond n) of tiled
// templates MT[tile16][channel][16]
__device__ __forceinline__ void quad_templates_listed(double *__restrict__ tpl, const double *__restrict__ model_t, int nxp,
                                                      const int *__restrict__ list, int g, int n)
{
	for (int e = threadIdx.x; e < nxp * 4; e += 256) {
		const int j = e >> 2, bb = e & 3;
		const int c = g + bb < n ? list[g + bb] : -1;
		const double m = c >= 0 ? model_t[((size_t) (c >> 4) * nxp + j) * 16 + (c & 15)] : 0.0;
		tpl[((size_t) (j >> 1) * 4 + bb) * 2 + (j & 1)] = m;
	}
}

// the sum of (candidate q, this quad's spectrum) over nst <= NST stages (nst wave-uniform)
template <int NST>
__device__ __forceinline__ double quad_sum(const double2 *__restrict__ tpl, int nst, int q, const double2 (&y)[NST])
{
	double acc = 0.0;
#pragma unroll
	for (int s = 0; s < NST; s++) {
		if (s < nst) {
			const double2 *m = tpl + (size_t) s * 16 + q;           // 4 channel pairs x 4 candidates per stage
			double d;
#define QUARTER(QQ) { const double2 mv = m[QQ * 4]; \
			d = mv.x - quad_bcast<QQ>(y[s].x); acc = fma(d, d, acc); \
			d = mv.y - quad_bcast<QQ>(y[s].y); acc = fma(d, d, acc); }
			QUARTER(0) QUARTER(1) QUARTER(2) QUARTER(3)
#undef QUARTER
		}
	}
	return acc;
}

// Accept test of lane (spectrum r of the tile, candidate cand_q, if has_q) and what leaves the kernel: the likelihoods
// that beat their threshold, and per candidate some spectrum of the tile accepts the flag, the ballot word and the
// stamp.  Wave w puts together the word of candidate cand_w (if has_w), the one the lanes q = w scored: lane l =
// spectrum l of the tile.  votes: [4 waves] in LDS; contains a workgroup barrier.
__device__ __forceinline__ void quad_vote(double L, double thr, bool has_q, int cand_q, bool has_w, int cand_w, int ntiles, int tile,
                                          int r, unsigned long long *votes, int *__restrict__ flags, int flag, const JointTrail &trail)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const bool beat = L > thr && has_q;
	const unsigned long long vote = __ballot(beat);                 // bit 4 i + q: spectrum wave * 16 + i, candidate q
	if (lane == 0) votes[wave] = vote;
	if (beat) trail.L[((size_t) cand_q * ntiles + tile) * 64 + r] = L;
	__syncthreads();
	const unsigned long long word = __ballot((votes[lane >> 4] >> (4 * (lane & 15) + wave)) & 1ull);
	if (has_w && word != 0ull && lane == 0) {
		const size_t at = (size_t) cand_w * ntiles + tile;
		flags[cand_w] = flag;
		trail.word[at] = word;
		trail.stamp_of[at] = trail.stamp;
	}
}

}  // namespace mdns
#endif
