// A tabulated template grid as the model of a run (mdns.h Part 12): the caller hands over the table once, the device
// interpolates it per candidate -- multilinear in the grid's parameters, linear along the templates' own abscissa at
// x / (1 + z), times an amplitude -- and the curves stay in device memory for the curve scoring kernels
// (mdns_curves.hip).
//
// Every value is the chain of single rounded fp64 operations that mdns.h Part 12 writes out; this file is compiled with
// -ffp-contract=off so that no multiply meets an add in an FMA, and the numpy statement
// (massivedatans_amd/tablemodel.py, TableModel.statement) reproduces the kernel bit for bit.  The kernel is a gather: the
// FMAs it gives up cost nothing.
//
// Two line-of-sight effects (MDNS_TABLE_EXTINCTION, MDNS_TABLE_BROADEN; mdns_table_create_los) take a second route:
// blend the corner rows at the template's knots, attenuate by 10 ** (ext[m] * E), broaden by a Gaussian in velocity,
// resample.  10 ** v is pow10_dd of mdns_pow10.h, which host and device compute identically, so the statement stays
// exact.  launch_table_curves chooses the route; a handle without the two flags runs k_table_curves as before.
#include "mdns_internal.h"
#include "mdns_pow10.h"
#include <cmath>
#include <vector>

namespace mdns {

// what the kernel takes by value (80-odd bytes of kernel arguments: scalar loads, no lane touches memory for them)
struct TableView {
	const double *x, *axes, *grid, *table;
	int nx, d, nw, ndim, flags;
	int pstride;                               // doubles between the rows of two candidates in `params` (>= ndim)
	int n[MDNS_TABLE_MAX_AXES];                // knots per axis
	int axis_at[MDNS_TABLE_MAX_AXES];          // where axis a begins in `axes`
	long long stride[MDNS_TABLE_MAX_AXES];     // doubles between neighbouring knots of axis a in `table`
};

// channels per workgroup, one per thread
static constexpr int kTableTile = MDNS_TABLE_TILE;

// the last knot <= v of knots[0 .. n-1] (ascending, n >= 2), capped at n - 2, for knots[0] <= v; 0 for a NaN
__device__ __forceinline__ int last_knot(const double *__restrict__ knots, int n, double v)
{
	int lo = 0, hi = n - 1;
	while (hi - lo > 1) {
		const int mid = (lo + hi) >> 1;
		if (knots[mid] <= v) lo = mid; else hi = mid;
	}
	return lo;
}

// the clamp of the statement, as comparisons: +-inf clamp, a NaN stays
__device__ __forceinline__ double clamp_to(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// grid (B, ceil(nx / kTableTile)): workgroup (b, tile) writes channels tile * kTableTile ... of candidate b.  The
// candidate's cell, fractions, 2^d corner weights and row offsets are made once per workgroup (threads 0 .. d-1 an axis
// each, then threads 0 .. 2^d - 1 a corner each) and read from LDS as broadcasts.  Thread t takes channel j: one binary
// search in the templates' abscissa, then per corner the pair T_c[k], T_c[k+1]; neighbouring threads have neighbouring
// (or equal) k, so a wave reads one contiguous window of every corner row.  Nothing a value is made of depends on B, on
// the candidate's place in the batch or on ldc.
__global__ __launch_bounds__(kTableTile) void k_table_curves(const TableView tv, const double *__restrict__ params, int B,
                                                              double *__restrict__ out, int ldc)
{
	__shared__ double s_f[MDNS_TABLE_MAX_AXES];
	__shared__ int s_i[MDNS_TABLE_MAX_AXES];
	__shared__ double s_w[1 << MDNS_TABLE_MAX_AXES];
	__shared__ long long s_off[1 << MDNS_TABLE_MAX_AXES];
	__shared__ int s_nan;
	const int b = blockIdx.x, tid = threadIdx.x, d = tv.d;
	if (b >= B) return;                                                   // (uniform over the workgroup)
	const double *__restrict__ p = params + (size_t) b * tv.pstride;
	if (tid < d) {
		const double *__restrict__ axis = tv.axes + tv.axis_at[tid];
		const int n = tv.n[tid];
		const double v = clamp_to(p[tid], axis[0], axis[n - 1]);
		const int i = last_knot(axis, n, v);
		s_i[tid] = i;
		s_f[tid] = (v - axis[i]) / (axis[i + 1] - axis[i]);
	} else if (tid == d) {
		int any = 0;
		for (int a = 0; a < tv.ndim; a++) any |= p[a] != p[a];
		s_nan = any;
	}
	__syncthreads();
	if (tid < (1 << d)) {
		double w = 1.0;
		long long off = 0;
		for (int a = 0; a < d; a++) {
			const int bit = (tid >> a) & 1;
			const double f = s_f[a];
			w = w * (bit ? f : 1.0 - f);
			off += (long long) (s_i[a] + bit) * tv.stride[a];
		}
		s_w[tid] = w;
		s_off[tid] = off;
	}
	__syncthreads();
	const int j = blockIdx.y * kTableTile + tid;
	if (j >= tv.nx) return;
	double *__restrict__ o = out + (size_t) b * ldc + j;
	if (s_nan) { *o = __builtin_nan(""); return; }
	double u = tv.x[j];
	if (tv.flags & MDNS_TABLE_REDSHIFT) u = u / (1.0 + p[d]);
	const int nw = tv.nw;
	u = clamp_to(u, tv.grid[0], tv.grid[nw - 1]);
	const int k = last_knot(tv.grid, nw, u);
	const double g0 = tv.grid[k];
	const double t = (u - g0) / (tv.grid[k + 1] - g0);
	double acc = 0.0;
	const int corners = 1 << d;
	for (int c = 0; c < corners; c++) {
		const double *__restrict__ T = tv.table + s_off[c] + k;
		const double lo = T[0], hi = T[1];
		acc = acc + s_w[c] * (lo + t * (hi - lo));
	}
	if (tv.flags & MDNS_TABLE_AMPLITUDE) acc = p[tv.ndim - 1] * acc;
	*o = acc;
}

// ---- the line-of-sight route (mdns.h Part 12, "with either new flag") ----

// what the kernels of this route take beside the TableView: the exponent per unit E at every template knot (or null),
// the quadrature widths of the knots (or null), and where E and s stand in a candidate's row (-1: not a parameter)
struct LosView {
	const double *ext, *delta;
	int at_e, at_s;
};

// a candidate whose whole row is NaN: a NaN in any parameter, an E that is not finite, an s that is not finite or < 0
__device__ __forceinline__ int los_row_is_nan(const TableView &tv, const LosView &lv, const double *__restrict__ p)
{
	int any = 0;
	for (int a = 0; a < tv.ndim; a++) any |= p[a] != p[a];
	if (lv.at_e >= 0) any |= !(fabs(p[lv.at_e]) < __builtin_inf());
	if (lv.at_s >= 0) any |= !(p[lv.at_s] >= 0.0 && p[lv.at_s] < __builtin_inf());
	return any;
}

// the setup k_table_curves makes per workgroup: cell and fractions (threads 0 .. d-1), the row's NaN flag (thread d),
// then weights and row offsets of the 2^d corners.  Needs a workgroup of 2^d threads at least; ends in a barrier.
__device__ __forceinline__ void los_corners(const TableView &tv, const LosView &lv, const double *__restrict__ p, double *s_f, int *s_i,
                                            double *s_w, long long *s_off, int *s_nan)
{
	const int tid = threadIdx.x, d = tv.d;
	if (tid < d) {
		const double *__restrict__ axis = tv.axes + tv.axis_at[tid];
		const int n = tv.n[tid];
		const double v = clamp_to(p[tid], axis[0], axis[n - 1]);
		const int i = last_knot(axis, n, v);
		s_i[tid] = i;
		s_f[tid] = (v - axis[i]) / (axis[i + 1] - axis[i]);
	} else if (tid == d) {
		*s_nan = los_row_is_nan(tv, lv, p);
	}
	__syncthreads();
	if (tid < (1 << d)) {
		double w = 1.0;
		long long off = 0;
		for (int a = 0; a < d; a++) {
			const int bit = (tid >> a) & 1;
			const double f = s_f[a];
			w = w * (bit ? f : 1.0 - f);
			off += (long long) (s_i[a] + bit) * tv.stride[a];
		}
		s_w[tid] = w;
		s_off[tid] = off;
	}
	__syncthreads();
}

// S_m of the statement: the corner rows blended at template knot m, then attenuated (E: the candidate's, ext: or null)
__device__ __forceinline__ double los_knot(const TableView &tv, const double *__restrict__ ext, double E, const double *s_w,
                                           const long long *s_off, int m)
{
	double S = 0.0;
	const int corners = 1 << tv.d;
	for (int c = 0; c < corners; c++) S = S + s_w[c] * tv.table[s_off[c] + m];
	if (ext) {
		const double q = clamp_to(ext[m] * E, -299.0, 299.0);
		S = S * mdns_pow10::pow10_dd(q);
	}
	return S;
}

// Extinction without broadening: a channel needs S at its two knots only, so this is k_table_curves' gather with the
// blend made at both knots and two 10 ** q per channel.  Same grid, same tile.
__global__ __launch_bounds__(kTableTile) void k_table_los_gather(const TableView tv, const LosView lv, const double *__restrict__ params, int B,
                                                                  double *__restrict__ out, int ldc)
{
	__shared__ double s_f[MDNS_TABLE_MAX_AXES];
	__shared__ int s_i[MDNS_TABLE_MAX_AXES];
	__shared__ double s_w[1 << MDNS_TABLE_MAX_AXES];
	__shared__ long long s_off[1 << MDNS_TABLE_MAX_AXES];
	__shared__ int s_nan;
	const int b = blockIdx.x, tid = threadIdx.x, d = tv.d;
	if (b >= B) return;                                                   // (uniform over the workgroup)
	const double *__restrict__ p = params + (size_t) b * tv.pstride;
	los_corners(tv, lv, p, s_f, s_i, s_w, s_off, &s_nan);
	const int j = blockIdx.y * kTableTile + tid;
	if (j >= tv.nx) return;
	double *__restrict__ o = out + (size_t) b * ldc + j;
	if (s_nan) { *o = __builtin_nan(""); return; }
	double u = tv.x[j];
	if (tv.flags & MDNS_TABLE_REDSHIFT) u = u / (1.0 + p[d]);
	const int nw = tv.nw;
	u = clamp_to(u, tv.grid[0], tv.grid[nw - 1]);
	const int k = last_knot(tv.grid, nw, u);
	const double g0 = tv.grid[k];
	const double t = (u - g0) / (tv.grid[k + 1] - g0);
	const double E = p[lv.at_e];
	const double lo = los_knot(tv, lv.ext, E, s_w, s_off, k), hi = los_knot(tv, lv.ext, E, s_w, s_off, k + 1);
	double acc = lo + t * (hi - lo);
	if (tv.flags & MDNS_TABLE_AMPLITUDE) acc = p[tv.ndim - 1] * acc;
	*o = acc;
}

// Stage 1 of the broadening route: S[b][m] for every template knot.  Grid (B, ceil(nw / kTableTile)), a knot per
// thread: neighbouring threads read neighbouring values of every corner row.  A NaN row writes nothing (no later stage
// reads it).
__global__ __launch_bounds__(kTableTile) void k_table_los_blend(const TableView tv, const LosView lv, const double *__restrict__ params, int B,
                                                                 double *__restrict__ S)
{
	__shared__ double s_f[MDNS_TABLE_MAX_AXES];
	__shared__ int s_i[MDNS_TABLE_MAX_AXES];
	__shared__ double s_w[1 << MDNS_TABLE_MAX_AXES];
	__shared__ long long s_off[1 << MDNS_TABLE_MAX_AXES];
	__shared__ int s_nan;
	const int b = blockIdx.x;
	if (b >= B) return;                                                   // (uniform over the workgroup)
	const double *__restrict__ p = params + (size_t) b * tv.pstride;
	los_corners(tv, lv, p, s_f, s_i, s_w, s_off, &s_nan);
	const int m = blockIdx.y * kTableTile + threadIdx.x;
	if (m >= tv.nw || s_nan) return;
	S[(size_t) b * tv.nw + m] = los_knot(tv, lv.ext, lv.ext ? p[lv.at_e] : 0.0, s_w, s_off, m);
}

// Stage 2: R[b][m] = the Gaussian-weighted mean of S[b][n] over the window of m (mdns.h Part 12, step 3).  A knot per
// thread: down from m to the first knot of its window, then ascending with the two running sums -- the statement's
// order.  Neighbouring threads have neighbouring windows, so their reads of S, grid and delta meet in the caches.  The
// window has no cap: a large s on a dense grid costs O(nw) per knot.
__global__ __launch_bounds__(kTableTile) void k_table_los_broaden(const TableView tv, const LosView lv, const double *__restrict__ params, int B,
                                                                   const double *__restrict__ S, double *__restrict__ R)
{
	const int b = blockIdx.x, m = blockIdx.y * kTableTile + threadIdx.x, nw = tv.nw;
	if (b >= B || m >= nw) return;
	const double *__restrict__ p = params + (size_t) b * tv.pstride;
	if (los_row_is_nan(tv, lv, p)) return;
	const double *__restrict__ Sb = S + (size_t) b * nw;
	const double s = p[lv.at_s];
	double r = Sb[m];
	if (s > 0.0) {
		const double *__restrict__ g = tv.grid;
		const double gm = g[m];
		int n = m;
		while (n > 0 && fabs(((g[n - 1] - gm) / gm) / s) <= MDNS_TABLE_BROADEN_CUT) n--;
		double num = 0.0, den = 0.0;
		for (; n < nw; n++) {
			const double dmn = ((g[n] - gm) / gm) / s;
			if (n > m && !(fabs(dmn) <= MDNS_TABLE_BROADEN_CUT)) break;
			const double K = mdns_pow10::pow10_dd((MDNS_TABLE_BROADEN_C * dmn) * dmn) * lv.delta[n];
			num = num + Sb[n] * K;
			den = den + K;
		}
		r = num / den;
	}
	R[(size_t) b * nw + m] = r;
}

// Stage 3: the curve read off R at u_j, k_table_curves' abscissa step on one row instead of 2^d
__global__ __launch_bounds__(kTableTile) void k_table_los_resample(const TableView tv, const LosView lv, const double *__restrict__ params, int B,
                                                                    const double *__restrict__ R, double *__restrict__ out, int ldc)
{
	const int b = blockIdx.x, j = blockIdx.y * kTableTile + threadIdx.x;
	if (b >= B || j >= tv.nx) return;
	const double *__restrict__ p = params + (size_t) b * tv.pstride;
	double *__restrict__ o = out + (size_t) b * ldc + j;
	if (los_row_is_nan(tv, lv, p)) { *o = __builtin_nan(""); return; }
	double u = tv.x[j];
	if (tv.flags & MDNS_TABLE_REDSHIFT) u = u / (1.0 + p[tv.d]);
	const int nw = tv.nw;
	u = clamp_to(u, tv.grid[0], tv.grid[nw - 1]);
	const int k = last_knot(tv.grid, nw, u);
	const double g0 = tv.grid[k];
	const double t = (u - g0) / (tv.grid[k + 1] - g0);
	const double *__restrict__ Rb = R + (size_t) b * nw + k;
	const double lo = Rb[0], hi = Rb[1];
	double acc = lo + t * (hi - lo);
	if (tv.flags & MDNS_TABLE_AMPLITUDE) acc = p[tv.ndim - 1] * acc;
	*o = acc;
}

static TableView table_view(const mdns_table *t, int pstride)
{
	TableView tv = {};
	tv.x = t->d_x.get(); tv.axes = t->d_axes.get(); tv.grid = t->d_grid.get(); tv.table = t->d_table.get();
	tv.nx = t->nx; tv.d = t->d; tv.nw = t->nw; tv.ndim = t->ndim; tv.flags = t->flags; tv.pstride = pstride;
	int at = 0;
	for (int a = 0; a < t->d; a++) { tv.n[a] = t->n[a]; tv.axis_at[a] = at; at += t->n[a]; }
	long long stride = t->nw;
	for (int a = t->d - 1; a >= 0; a--) { tv.stride[a] = stride; stride *= t->n[a]; }
	return tv;
}

static LosView los_view(const mdns_table *t)
{
	LosView lv = {};
	const bool e = t->flags & MDNS_TABLE_EXTINCTION, s = t->flags & MDNS_TABLE_BROADEN;
	lv.ext = e ? t->d_ext.get() : nullptr;
	lv.delta = s ? t->d_delta.get() : nullptr;
	lv.at_e = e ? t->d + ((t->flags & MDNS_TABLE_REDSHIFT) ? 1 : 0) : -1;
	lv.at_s = s ? t->d + ((t->flags & MDNS_TABLE_REDSHIFT) ? 1 : 0) + (e ? 1 : 0) : -1;
	return lv;
}

// the one place that chooses the route: neither new flag k_table_curves, extinction alone the gather with two knots,
// broadening the three stages through the handle's grow-only S and R.  pstride: doubles between the rows of two
// candidates (>= t->ndim; a sum model hands over a slice of wider rows, mdns_sum.hip); no value depends on it
bool launch_table_curves(mdns_table *t, const double *d_params, int B, double *d_out, int ldc, int pstride)
{
	Context *c = ctx();
	if (!c) return false;
	if (B <= 0) return true;
	const dim3 grid((unsigned) B, (unsigned) ((t->nx + kTableTile - 1) / kTableTile));
	const TableView tv = table_view(t, pstride);
	if (!(t->flags & (MDNS_TABLE_EXTINCTION | MDNS_TABLE_BROADEN))) {
		hipLaunchKernelGGL(k_table_curves, grid, dim3(kTableTile), 0, c->stream, tv, d_params, B, d_out, ldc);
		return launched("k_table_curves");
	}
	const LosView lv = los_view(t);
	if (!(t->flags & MDNS_TABLE_BROADEN)) {
		hipLaunchKernelGGL(k_table_los_gather, grid, dim3(kTableTile), 0, c->stream, tv, lv, d_params, B, d_out, ldc);
		return launched("k_table_los_gather");
	}
	const size_t knots = (size_t) B * t->nw;
	// (a refused growth leaves the buffer empty and the handle as it was: the next call asks again)
	if (!t->d_S.fit(knots) || !t->d_R.fit(knots)) return false;
	const dim3 wgrid((unsigned) B, (unsigned) ((t->nw + kTableTile - 1) / kTableTile));
	hipLaunchKernelGGL(k_table_los_blend, wgrid, dim3(kTableTile), 0, c->stream, tv, lv, d_params, B, t->d_S.get());
	if (!launched("k_table_los_blend")) return false;
	hipLaunchKernelGGL(k_table_los_broaden, wgrid, dim3(kTableTile), 0, c->stream, tv, lv, d_params, B, t->d_S.get(), t->d_R.get());
	if (!launched("k_table_los_broaden")) return false;
	hipLaunchKernelGGL(k_table_los_resample, grid, dim3(kTableTile), 0, c->stream, tv, lv, d_params, B, t->d_R.get(), d_out, ldc);
	return launched("k_table_los_resample");
}

bool launch_table_curves(mdns_table *t, const double *d_params, int B, double *d_out, int ldc)
{
	return launch_table_curves(t, d_params, B, d_out, ldc, t->ndim);
}

}  // namespace mdns

using namespace mdns;

// knots[0 .. n-1] finite and strictly increasing; else the error names `what` and the index
static bool knots_ok(const char *who, const double *knots, int n, const char *what, int axis)
{
	for (int i = 0; i < n; i++) {
		if (!std::isfinite(knots[i])) {
			if (axis >= 0) set_error("%s: axis %d: knot %d = %g is not finite", who, axis, i, knots[i]);
			else set_error("%s: %s[%d] = %g is not finite", who, what, i, knots[i]);
			return false;
		}
		if (i > 0 && !(knots[i] > knots[i - 1])) {
			if (axis >= 0) set_error("%s: axis %d is not strictly increasing at knot %d", who, axis, i);
			else set_error("%s: %s is not strictly increasing at [%d]", who, what, i);
			return false;
		}
	}
	return true;
}

// every create entry (mdns_sum_add_table of mdns_sum.hip too): `known` the flag bits `who` takes, `ext` null for
// mdns_table_create.  Every rule of the statement, on the host copies, before the device is asked for anything
mdns_table *mdns::table_create(const char *who, int known, const double *x, int nx, int d, const int *n, const double *axes, int nw,
                                const double *grid, const double *table, int flags, const double *ext)
{
	if (!x || !n || !axes || !grid || !table) { set_error("%s: null argument", who); return nullptr; }
	if (nx < 1 || nx > MDNS_TABLE_MAX_NX) { set_error("%s: nx=%d: 1 to %d channels", who, nx, MDNS_TABLE_MAX_NX); return nullptr; }
	if (d < 1 || d > MDNS_TABLE_MAX_AXES) { set_error("%s: d=%d: 1 to %d axes", who, d, MDNS_TABLE_MAX_AXES); return nullptr; }
	if (flags & ~known) { set_error("%s: flags=%d: unknown bits", who, flags); return nullptr; }
	int ndim = d;
	for (int bit = 1; bit <= MDNS_TABLE_BROADEN; bit <<= 1) ndim += (flags & bit) ? 1 : 0;
	if (ndim > MDNS_MAX_DIM) { set_error("%s: %d parameters > %d", who, ndim, MDNS_MAX_DIM); return nullptr; }
	if (nw < 2) { set_error("%s: nw=%d: the templates need 2 knots at least", who, nw); return nullptr; }
	long long elems = nw, knots = 0;
	for (int a = 0; a < d; a++) {
		if (n[a] < 2) { set_error("%s: axis %d has %d knots: 2 at least", who, a, n[a]); return nullptr; }
		knots += n[a];
		elems *= n[a];                                                // (<= 2^31 * 2^31 before the test: no overflow)
		if (elems > MDNS_TABLE_MAX_ELEMS || knots > MDNS_TABLE_MAX_ELEMS) {
			set_error("%s: the table is too large: more than %lld values up to axis %d", who, (long long) MDNS_TABLE_MAX_ELEMS, a);
			return nullptr;
		}
	}
	for (int j = 0; j < nx; j++)
		if (!std::isfinite(x[j])) { set_error("%s: x[%d] = %g is not finite", who, j, x[j]); return nullptr; }
	const double *axis = axes;
	for (int a = 0; a < d; a++) {
		if (!knots_ok(who, axis, n[a], "axis", a)) return nullptr;
		axis += n[a];
	}
	if (!knots_ok(who, grid, nw, "grid", -1)) return nullptr;
	for (long long i = 0; i < elems; i++)
		if (!std::isfinite(table[i])) { set_error("%s: table[%lld] = %g is not finite", who, i, table[i]); return nullptr; }
	const bool extinction = flags & MDNS_TABLE_EXTINCTION, broaden = flags & MDNS_TABLE_BROADEN;
	if (extinction) {
		if (!ext) { set_error("%s: null ext with MDNS_TABLE_EXTINCTION", who); return nullptr; }
		for (int m = 0; m < nw; m++)
			if (!std::isfinite(ext[m])) { set_error("%s: ext[%d] = %g is not finite", who, m, ext[m]); return nullptr; }
	}
	if (broaden && !(grid[0] > 0)) { set_error("%s: grid[0] = %g: MDNS_TABLE_BROADEN needs a grid > 0", who, grid[0]); return nullptr; }
	// the quadrature widths of the statement's broadening sum, made here once (tablemodel.py makes the same)
	std::vector<double> delta;
	if (broaden) {
		delta.resize((size_t) nw);
		for (int m = 1; m < nw - 1; m++) delta[m] = (grid[m + 1] - grid[m - 1]) * 0.5;
		delta[0] = (grid[1] - grid[0]) * 0.5;
		delta[nw - 1] = (grid[nw - 1] - grid[nw - 2]) * 0.5;
	}
	Context *c = ctx();
	if (!c) return nullptr;
	mdns_table *t = new mdns_table();
	t->nx = nx; t->d = d; t->nw = nw; t->ndim = ndim; t->flags = flags;
	for (int a = 0; a < d; a++) t->n[a] = n[a];
	// (pageable sources; the synchronise below lets the caller's arrays go)
	const bool ok =
	    t->d_x.make((size_t) nx) && t->d_axes.make((size_t) knots) && t->d_grid.make((size_t) nw) && t->d_table.make((size_t) elems) &&
	    MDNS_HIP(hipMemcpyAsync(t->d_x.get(), x, (size_t) nx * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipMemcpyAsync(t->d_axes.get(), axes, (size_t) knots * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipMemcpyAsync(t->d_grid.get(), grid, (size_t) nw * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    MDNS_HIP(hipMemcpyAsync(t->d_table.get(), table, (size_t) elems * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	    (!extinction || (t->d_ext.make((size_t) nw) &&
	                     MDNS_HIP(hipMemcpyAsync(t->d_ext.get(), ext, (size_t) nw * sizeof(double), hipMemcpyHostToDevice, c->stream)))) &&
	    (!broaden || (t->d_delta.make((size_t) nw) &&
	                  MDNS_HIP(hipMemcpyAsync(t->d_delta.get(), delta.data(), (size_t) nw * sizeof(double), hipMemcpyHostToDevice, c->stream)))) &&
	    MDNS_HIP(hipStreamSynchronize(c->stream));
	if (!ok) { mdns_table_destroy(t); return nullptr; }               // (the owners free what was made)
	return t;
}

extern "C" mdns_table *mdns_table_create(const double *x, int nx, int d, const int *n, const double *axes, int nw, const double *grid,
                                         const double *table, int flags)
{
	return table_create("mdns_table_create", MDNS_TABLE_REDSHIFT | MDNS_TABLE_AMPLITUDE, x, nx, d, n, axes, nw, grid, table, flags, nullptr);
}

extern "C" mdns_table *mdns_table_create_los(const double *x, int nx, int d, const int *n, const double *axes, int nw, const double *grid,
                                             const double *table, int flags, const double *ext)
{
	return table_create("mdns_table_create_los", MDNS_TABLE_REDSHIFT | MDNS_TABLE_AMPLITUDE | MDNS_TABLE_EXTINCTION | MDNS_TABLE_BROADEN, x, nx,
	                    d, n, axes, nw, grid, table, flags, ext);
}

extern "C" void mdns_table_destroy(mdns_table *t)
{
	if (!t) return;
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	delete t;
}

extern "C" int mdns_table_nparams(const mdns_table *t) { return t ? t->ndim : -1; }
extern "C" int mdns_table_nx(const mdns_table *t) { return t ? t->nx : -1; }

// what both forms check first; 1: refused, 0: go on, -1: nothing to do
static int table_batch_check(const mdns_table *t, const void *params, int B, const void *out, int ldc, const char *who)
{
	if (!ctx()) return 1;
	if (!t) { set_error("%s: null table handle", who); return 1; }
	if (B < 0 || ldc < t->nx) { set_error("%s: bad sizes B=%d ldc=%d (nx=%d)", who, B, ldc, t->nx); return 1; }
	if (B == 0) return -1;
	if (!params || !out) { set_error("%s: null argument", who); return 1; }
	return 0;
}

extern "C" int mdns_table_curves_batch_dev(mdns_table *t, const double *d_params, int B, double *d_out, int ldc)
{
	const int rc = table_batch_check(t, d_params, B, d_out, ldc, "mdns_table_curves_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_table_curves(t, d_params, B, d_out, ldc) ? 0 : 1;
}

extern "C" int mdns_table_curves_batch(mdns_table *t, const double *params, int B, double *out)
{
	Context *c = ctx();
	const int rc = table_batch_check(t, params, B, out, t ? t->nx : 0, "mdns_table_curves_batch");
	if (rc != 0) return rc > 0;
	const size_t np = (size_t) B * t->ndim, no = (size_t) B * t->nx;
	if (!t->d_params.fit(np) || !t->d_out.fit(no)) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(t->d_params.get(), params, np * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (!launch_table_curves(t, t->d_params.get(), B, t->d_out.get(), t->nx)) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(out, t->d_out.get(), no * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
