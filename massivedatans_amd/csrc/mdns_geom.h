// What the RadFriends geometry kernels share (K3..K6 in mdns_neighbors.hip and mdns_k6sort.hip, k_box_count in
// mdns_chain.hip): the squared distance, the reductions, the steps of K6 that more than one kernel takes, the end of a
// radius computation and the end of a membership count -- one statement each.
//
// RELIES ON -ffp-contract=off: the squared distance keeps multiply and add separate (cneighbors.c:55-58).  Every
// translation unit that includes this header is compiled with that flag and says `#pragma clang fp contract(off)`
// itself; the pragma below covers the functions defined here.
#pragma once
#include "mdns_internal.h"

#ifdef __HIPCC__
#pragma clang fp contract(off)

namespace mdns {

// ---- launch switches over the compiled dimensions ---------------------------------------------------------------
static constexpr int kMaxRegDim = 8;        // dimensions kept in registers
// 1..8 in registers, 0 = runtime ndim (generic path)
#define MDNS_DIM_SWITCH(ndim, LAUNCH) \
	switch ((ndim) <= kMaxRegDim ? (ndim) : 0) { \
	case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; \
	case 4: LAUNCH(4); break; case 5: LAUNCH(5); break; case 6: LAUNCH(6); break; \
	case 7: LAUNCH(7); break; case 8: LAUNCH(8); break; default: LAUNCH(0); break; }
// kernels that exist for 1..5 dimensions only (the caller has checked the range)
#define MDNS_DIM5_SWITCH(ndim, LAUNCH) \
	switch (ndim) { case 1: LAUNCH(1); break; case 2: LAUNCH(2); break; case 3: LAUNCH(3); break; \
	                case 4: LAUNCH(4); break; default: LAUNCH(5); break; }

// ---- squared distance: from 0 over the dimensions in ascending order, separate multiply and add ------------------
__device__ __forceinline__ double sq_distance(const double *a, const double *b, int ndim)
{
	double acc = 0.0;
	for (int k = 0; k < ndim; k++) {
		const double diff = a[k] - b[k];
		acc = acc + diff * diff;
	}
	return acc;
}

template <int D>
__device__ __forceinline__ double sq_distance_fixed(const double *a, const double (&c)[D])
{
	double acc = 0.0;
#pragma unroll
	for (int k = 0; k < D; k++) {
		const double diff = a[k] - c[k];
		acc = acc + diff * diff;
	}
	return acc;
}

// ---- reductions ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
	return v;
}
__device__ __forceinline__ double wave_min(double v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
	return v;
}

// min(a, b) where b may be a QUIET NaN meaning "not a candidate": v_min_f64 returns the other
// operand for a quiet NaN.  Written as asm so that the compiler does not put a canonicalising
// v_max_f64 in front of every use (it cannot know the operand is already quiet).
__device__ __forceinline__ double min_or_skip(double a, double b)
{
	double r;
	asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
	return r;
}

// non-negative doubles order like their bit patterns
__device__ __forceinline__ void atomic_max_nonneg(double *addr, double v)
{
	atomicMax(reinterpret_cast<unsigned long long *>(addr), (unsigned long long) __double_as_longlong(v));
}

// ---- K6 with a wave-uniform member: the pair step -----------------------------------------------------------------
// The squared distance d of (this lane's point, one member) offered to the RT rounds; bit b of m (a SCALAR: the member
// is the same for every lane of the wave) says whether the member is chosen in round b.  Per round  v_max_f64 t, d, S
// with S = -inf where the member is chosen (t = d) and +inf where it is not (t = +inf), then  v_min_f64 nearest, t.
// (tried: `if (m >> b & 1u) nearest[b] = min(nearest[b], d)` -- a scalar branch around ONE
// v_min_f64, 14 vector instructions per step instead of 28: 47.7 / 124 / 409 / 2198 us at
// 5 000 / 9 000 / 20 000 / 50 000 points against 51 / 111 / 400 / 2130 -- the ten
// s_bitcmp1 + s_cbranch pairs per step cost what the skipped instructions save)
template <int RT>
__device__ __forceinline__ void offer_rounds(double (&nearest)[RT], double d, unsigned m)
{
	const double PINF = __longlong_as_double(0x7ff0000000000000LL), NINF = __longlong_as_double((long long) 0xfff0000000000000ULL);
#pragma unroll
	for (int b = 0; b < RT; b++) {
		const double S = (m >> b & 1u) ? NINF : PINF;             // scalar: s_bitcmp1 + s_cselect_b64
		// (written as asm: left to itself the compiler turns max(d, +-inf) into two
		// v_cndmask_b32 per round -- three vector instructions instead of two; so does the
		// quiet-NaN form d.hi | 0x7ff80000 of the classic kernel with a scalar mask: it needs a
		// copy of d.lo per round to form the register pair)
		double t;
		asm("v_max_f64 %0, %1, %2" : "=v"(t) : "v"(d), "s"(S));
		nearest[b] = min_or_skip(nearest[b], t);
	}
}

// ---- K6 split over member chunks: the merge -------------------------------------------------------------------------
// part[y][K][RT] holds, per member chunk y, every point's nearest chosen member of that chunk.  A workgroup of 256
// threads takes the 64 points from `first_point` on: the min over the chunks, then per round the max over the
// LEFT-OUT points with index >= 1 into round_sq (cneighbors.c:160-168: a point chosen in a round does not contribute
// to it, and the reference's max loop starts at 1, so the pool's point 0 never does).  Rounds >= nb are not there.
// Four lanes per point, each with every fourth chunk (one lane per point walking all chunks: 12 us at 5 000 points in
// 20 workgroups -- a chain of dependent row reads).  wmax: LDS of the caller's.
// AGENT_LOADS: `part` was written by other workgroups of THIS launch (agent-scope stores: see handover_release); false:
// by an earlier launch, plain loads.
template <int RT, bool AGENT_LOADS>
__device__ __forceinline__ void merge_chunks(const double *__restrict__ part, int K, int ny, int first_point,
                                             const unsigned *__restrict__ mask, int nb, double *__restrict__ round_sq,
                                             double (&wmax)[4][RT])
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	const int i = first_point + (threadIdx.x >> 2), yq = threadIdx.x & 3;
	double v[RT];
#pragma unroll
	for (int b = 0; b < RT; b++) v[b] = 0.0;
	const bool counts = i < K && i >= 1;
	if (counts) {
#pragma unroll
		for (int b = 0; b < RT; b++) v[b] = 1e300;
		for (int y = yq; y < ny; y += 4) {
			const double *row = part + ((size_t) y * K + i) * RT;
#pragma unroll
			for (int b = 0; b < RT; b++)
				v[b] = fmin(v[b], AGENT_LOADS ? __hip_atomic_load(row + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : row[b]);
		}
	}
#pragma unroll
	for (int b = 0; b < RT; b++) {
		v[b] = fmin(v[b], __shfl_xor(v[b], 1, 64));
		v[b] = fmin(v[b], __shfl_xor(v[b], 2, 64));
	}
	if (counts) {
		const unsigned m = mask[i];
#pragma unroll
		for (int b = 0; b < RT; b++) if (b >= nb || (m >> b & 1u)) v[b] = 0.0;     // chosen points do not contribute
	}
#pragma unroll
	for (int b = 0; b < RT; b++) {
		const double w = wave_max(v[b]);
		if (lane == 0) wmax[wv][b] = w;
	}
	__syncthreads();
	if (threadIdx.x < RT && threadIdx.x < nb) {
		const double w = fmax(fmax(wmax[0][threadIdx.x], wmax[1][threadIdx.x]), fmax(wmax[2][threadIdx.x], wmax[3][threadIdx.x]));
		if (w > 0.0) atomic_max_nonneg(round_sq + threadIdx.x, w);
	}
}

// ---- the end of a radius computation ----------------------------------------------------------------------------------
// Radius and membership threshold of a region, on the device: radius = sqrt(max_b round_sq[b])
// (cneighbors.c:160-174; sqrt after the max, monotone) and thresh = the smallest double T
// with sqrt(T) >= radius, so that  sqrt(d) < radius  <=>  d < T  (cneighbors.c:88,109).  Same
// bisection over bit patterns as mdns::sqrt_threshold on the host; hipcc's sqrt(double) is
// correctly rounded (verified bit for bit against the host on 1.6e7 inputs, and the parity
// tests compare both paths), so the two agree exactly.  Run by one lane of the last workgroup
// of a radius computation (normally ~15 square roots).
__device__ __forceinline__ void radius_and_threshold(double max_sq, double &radius, double &thresh)
{
	const double r = sqrt(max_sq);     // sqrt after the max: same number, sqrt is monotone
	double T;
	if (!(r > 0.0)) T = 0.0;                       // nothing is strictly within a zero radius
	else if (r == __longlong_as_double(0x7ff0000000000000LL)) T = r;
	else {
		// T lies within a few ulps of r*r: walk there, and keep the full bisection for the
		// cases where r*r leaves the normal range or the walk does not settle
		const double t0 = r * r;
		unsigned long long u = (unsigned long long) __double_as_longlong(t0);
		bool settled = false;
		if (t0 > 1e-300 && t0 < 1e300) {
			int guard = 0;
			while (sqrt(__longlong_as_double((long long) u)) < r && guard < 8) { u++; guard++; }
			while (guard < 16 && sqrt(__longlong_as_double((long long) (u - 1))) >= r) { u--; guard++; }
			settled = guard < 16 && sqrt(__longlong_as_double((long long) u)) >= r &&
			          sqrt(__longlong_as_double((long long) (u - 1))) < r;
		}
		if (!settled) {
			unsigned long long lo = 0, hi = 0x7ff0000000000000ULL;
			while (hi - lo > 1) {
				const unsigned long long mid = lo + (hi - lo) / 2;
				if (sqrt(__longlong_as_double((long long) mid)) >= r) hi = mid; else lo = mid;
			}
			u = hi;
		}
		T = __longlong_as_double((long long) u);
	}
	radius = r;
	thresh = T;
}

// Every thread of every workgroup of the launch that finishes a radius computation calls this once its own maxima
// are in rounds[0, nrounds) (atomic max); workgroups of 256 or 512 threads, gridDim.x of them.  The workgroup that
// gets here LAST -- it alone knows that all per-round maxima are final -- turns them into {radius, threshold}: once
// into device memory for the membership kernel that follows in stream order, once into mapped host memory, where the
// host polls `seq` (written last).  fin.counter == nullptr: this launch does not finish the computation.
// Two contracts, stated here and nowhere else:
//   - a finishing computation leaves its round slots ZERO: the next one raises them with atomic max and no launch
//     clears them (nobody else reads them any more when they are reset here);
//   - fin.counter is zero outside a launch: the last workgroup resets it for the next one (stream order).
// Why handover_release + barrier + ticket suffices: the maxima are atomics and the ticket is an atomic, all at agent
// scope, so they act on memory itself; each wave waits for its own to be acknowledged, the barrier collects the waves
// of the workgroup, and only then does one lane take the ticket -- whoever draws the last ticket therefore comes after
// every maximum of every workgroup, and reads them with agent-scope loads.  No cache is written back or invalidated.
__device__ __forceinline__ void finish_radius(const BootstrapFinish &fin, double *rounds, int nrounds)
{
	if (!fin.counter) return;
	handover_release();                                   // this wave's atomics before the workgroup's ticket
	__syncthreads();
	if (threadIdx.x >= 64) return;
	const int lane = threadIdx.x;
	unsigned ticket = 0;
	if (lane == 0) ticket = atomicAdd(fin.counter, 1u);
	if (__shfl(ticket, 0, 64) != gridDim.x - 1) return;
	handover_acquire();
	double best = 0.0;
	for (int b = lane; b < nrounds; b += 64)
		best = fmax(best, __hip_atomic_load(rounds + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
	best = wave_max(best);
	for (int b = lane; b < nrounds; b += 64) rounds[b] = 0.0;
	if (lane != 0) return;
	double radius, thresh;
	radius_and_threshold(best, radius, thresh);
	fin.d_res->radius = radius;
	fin.d_res->thresh = thresh;
	*fin.counter = 0;
	mail_store(&fin.h_res->radius, radius);
	mail_store(&fin.h_res->thresh, thresh);
	mail_raise(&fin.h_res->seq, fin.seq);
}

// ---- the end of a membership count (k_count_within, k_box_count) ------------------------------------------------------
// A wave is PTS points x 64 / PTS member slices (lane = point + PTS * slice), a workgroup 4 such waves on the same
// points.  Sum of `hits` over the slices of a wave, then over the waves through part[4][PTS] (LDS): the total of
// point `lane` -- for the lanes < PTS of wave 0, which are the ones that store it.  Every thread calls (barrier).
template <int PTS>
__device__ __forceinline__ int slice_total(int hits, int *part)
{
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, pt = lane % PTS;
#pragma unroll
	for (int off = PTS; off < 64; off <<= 1) hits += __shfl_xor(hits, off, 64);
	if (lane < PTS) part[wv * PTS + pt] = hits;
	__syncthreads();
	return (part[pt] + part[PTS + pt]) + (part[2 * PTS + pt] + part[3 * PTS + pt]);
}

// The totals went to host memory mapped into the device as system-scope stores by wave 0 (mail_store): once every
// workgroup's stores are out -- waited for, not fenced: see handover_release -- the last of the launch's
// `nworkgroups` to get here raises `seq` for the polling host and leaves the ticket zero for the next launch
// (stream order).  Every thread calls; mail.seq_at == nullptr: nobody polls.
__device__ __forceinline__ void count_mail_raise(const CountMail &mail, unsigned nworkgroups)
{
	if (!mail.seq_at) return;
	if (threadIdx.x < 64) handover_release();                  // (only wave 0 stored)
	__syncthreads();
	if (threadIdx.x != 0) return;
	const int done = atomicAdd(mail.ticket, 1);
	if (done != (int) nworkgroups - 1) return;
	__hip_atomic_store(mail.ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	mail_raise(mail.seq_at, mail.seq);
}

}  // namespace mdns
#endif
