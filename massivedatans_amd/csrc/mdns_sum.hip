// A sum of components as the model of a run (mdns.h Part 14): up to MDNS_SUM_MAX_COMPONENTS tables (Part 12), power
// laws and Gaussian lines, a common attenuation factor optional, evaluated on the device from the candidates'
// parameters; the curves stay in device memory for the curve scoring kernels (mdns_curves.hip).
//
// Every value is the chain of single rounded fp64 operations that mdns.h Part 14 writes out; this file is compiled with
// -ffp-contract=off so that no multiply meets an add in an FMA, 10 ** v is pow10_dd of mdns_pow10.h, which host and
// device compute identically, and the numpy statement (massivedatans_amd/summodel.py, SumModel.statement) reproduces the
// kernel bit for bit.
//
// Two passes on the library stream: launch_table_curves (mdns_table.hip) once per table component, reading its slice
// of the candidates' rows and writing its slice of the handle's scratch [tables][B][nx]; then ONE k_sum_curves, which
// computes the analytic components where it stands and reads the tables' values from the scratch.
#include "mdns_internal.h"
#include "mdns_pow10.h"
#include <cmath>

namespace mdns {

// what the kernel takes by value (224 bytes of kernel arguments: scalar loads, no lane touches memory for them)
struct SumComp {
	const double *ptr;         // TABLE: the component's curves [B][nx] in the scratch; POWERLAW: lx [nx]; GAUSS: unused
	int kind, at;              // MDNS_SUM_*; where the component's parameters begin in a row
	int attenuated, pad;
};
struct SumView {
	const double *x, *att;     // att: nullptr without an attenuation
	int nx, ndim, ncomp, pad;
	SumComp c[MDNS_SUM_MAX_COMPONENTS];
};

// bins per workgroup, one per thread
static constexpr int kSumTile = MDNS_TABLE_TILE;

// the clamp of the statement, as comparisons: +-inf clamp, a NaN stays
__device__ __forceinline__ double sum_clamp(double v) { return v < -299.0 ? -299.0 : (v > 299.0 ? 299.0 : v); }
__device__ __forceinline__ int not_finite(double v) { return !(fabs(v) < __builtin_inf()); }

// grid (B, ceil(nx / kSumTile)): workgroup (b, tile) writes bins tile * kSumTile ... of candidate b.  Thread 0 makes the
// row's NaN flag (a NaN anywhere, an analytic parameter or N that is not finite, a sigma that is not > 0), which goes
// through LDS behind a barrier; then thread t takes bin j and walks the components in their order.  The candidate's
// parameters are the same for the whole workgroup: scalar loads.  Nothing a value is made of depends on B, on the
// candidate's place in the batch or on ldc.
__global__ __launch_bounds__(kSumTile) void k_sum_curves(const SumView sv, const double *__restrict__ params, int B,
                                                          double *__restrict__ out, int ldc)
{
	__shared__ int s_nan;
	const int b = blockIdx.x, tid = threadIdx.x;
	if (b >= B) return;                                                   // (uniform over the workgroup)
	const double *__restrict__ p = params + (size_t) b * sv.ndim;
	if (tid == 0) {
		int any = 0;
		for (int a = 0; a < sv.ndim; a++) any |= p[a] != p[a];
		for (int c = 0; c < sv.ncomp; c++) {
			const int at = sv.c[c].at;
			if (sv.c[c].kind == MDNS_SUM_POWERLAW) any |= not_finite(p[at]) | not_finite(p[at + 1]);
			else if (sv.c[c].kind == MDNS_SUM_GAUSS)
				any |= not_finite(p[at]) | not_finite(p[at + 1]) | !(p[at + 2] > 0.0 && p[at + 2] < __builtin_inf());
		}
		if (sv.att) any |= not_finite(p[sv.ndim - 1]);
		s_nan = any;
	}
	__syncthreads();
	const int j = blockIdx.y * kSumTile + tid;
	if (j >= sv.nx) return;
	double *__restrict__ o = out + (size_t) b * ldc + j;
	if (s_nan) { *o = __builtin_nan(""); return; }
	const double xj = sv.x[j];
	double a = 0.0, u = 0.0;
	for (int c = 0; c < sv.ncomp; c++) {
		const SumComp &sc = sv.c[c];
		double v;
		if (sc.kind == MDNS_SUM_TABLE) {
			v = sc.ptr[(size_t) b * sv.nx + j];
		} else if (sc.kind == MDNS_SUM_POWERLAW) {
			double q = p[sc.at + 1] * sc.ptr[j];
			q = p[sc.at] - q;
			v = mdns_pow10::pow10_dd(sum_clamp(q));
		} else {
			const double d = (xj - p[sc.at + 1]) / p[sc.at + 2];
			const double q = (MDNS_TABLE_BROADEN_C * d) * d;
			v = p[sc.at] * mdns_pow10::pow10_dd(sum_clamp(q));
		}
		if (sc.attenuated) a = a + v; else u = u + v;
	}
	if (sv.att) {
		const double q = sum_clamp(sv.att[j] * p[sv.ndim - 1]);
		a = a * mdns_pow10::pow10_dd(q);
	}
	*o = a + u;
}

bool sum_ready(const mdns_sum *m, const char *who)
{
	if (!m) { set_error("%s: null sum handle", who); return false; }
	if (m->ncomp < 1) { set_error("%s: a model without components", who); return false; }
	return true;
}

bool launch_sum_curves(mdns_sum *m, const double *d_params, int B, double *d_out, int ldc)
{
	Context *c = ctx();
	if (!c) return false;
	m->used = 1;
	if (B <= 0) return true;
	const int ndim = m->ndim();
	int tables = 0;
	for (int k = 0; k < m->ncomp; k++) tables += m->kind[k] == MDNS_SUM_TABLE;
	const size_t slice = (size_t) B * m->nx;
	// (a refused growth leaves the buffer empty and the handle as it was: the next call asks again)
	if (tables && !m->d_tcurves.fit(slice * tables)) return false;
	SumView sv = {};
	sv.x = m->d_x.get();
	sv.att = m->has_att ? m->d_att.get() : nullptr;
	sv.nx = m->nx; sv.ndim = ndim; sv.ncomp = m->ncomp;
	int t = 0;
	for (int k = 0; k < m->ncomp; k++) {
		SumComp &sc = sv.c[k];
		sc.kind = m->kind[k];
		sc.at = m->at[k];
		sc.attenuated = m->has_att ? m->attenuated[k] : 1;                // (without an attenuation one sum holds them all)
		sc.ptr = nullptr;
		if (sc.kind == MDNS_SUM_POWERLAW) sc.ptr = m->d_lx[k].get();
		if (sc.kind != MDNS_SUM_TABLE) continue;
		double *mine = m->d_tcurves.get() + slice * t++;
		if (!launch_table_curves(m->table[k], d_params + sc.at, B, mine, m->nx, ndim)) return false;
		sc.ptr = mine;
	}
	const dim3 grid((unsigned) B, (unsigned) ((m->nx + kSumTile - 1) / kSumTile));
	hipLaunchKernelGGL(k_sum_curves, grid, dim3(kSumTile), 0, c->stream, sv, d_params, B, d_out, ldc);
	return launched("k_sum_curves");
}

}  // namespace mdns

using namespace mdns;

extern "C" mdns_sum *mdns_sum_create(const double *x, int nx)
{
	const char *who = "mdns_sum_create";
	if (!x) { set_error("%s: null argument", who); return nullptr; }
	if (nx < 1 || nx > MDNS_TABLE_MAX_NX) { set_error("%s: nx=%d: 1 to %d bins", who, nx, MDNS_TABLE_MAX_NX); return nullptr; }
	for (int j = 0; j < nx; j++)
		if (!std::isfinite(x[j])) { set_error("%s: x[%d] = %g is not finite", who, j, x[j]); return nullptr; }
	Context *c = ctx();
	if (!c) return nullptr;
	mdns_sum *m = new mdns_sum();
	m->nx = nx;
	m->x.assign(x, x + nx);
	// (a pageable source; the synchronise lets the caller's array go)
	const bool ok = m->d_x.make((size_t) nx) &&
	                MDNS_HIP(hipMemcpyAsync(m->d_x.get(), x, (size_t) nx * sizeof(double), hipMemcpyHostToDevice, c->stream)) &&
	                MDNS_HIP(hipStreamSynchronize(c->stream));
	if (!ok) { delete m; return nullptr; }
	return m;
}

extern "C" void mdns_sum_destroy(mdns_sum *m)
{
	if (!m) return;
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	for (int k = 0; k < m->ncomp; k++) delete m->table[k];               // (the stream has drained: the owners may free)
	delete m;
}

extern "C" int mdns_sum_nparams(const mdns_sum *m) { return m ? m->ndim() : -1; }
extern "C" int mdns_sum_nx(const mdns_sum *m) { return m ? m->nx : -1; }
extern "C" int mdns_sum_ncomponents(const mdns_sum *m) { return m ? m->ncomp : -1; }

// what every add entry and mdns_sum_set_attenuation refuse first; `more`: the parameters the call would add
static bool sum_open(const mdns_sum *m, const char *who, int more, bool component)
{
	if (!m) { set_error("%s: null sum handle", who); return false; }
	if (m->used) { set_error("%s: the model is fixed at its first use", who); return false; }
	if (component && m->ncomp >= MDNS_SUM_MAX_COMPONENTS) {
		set_error("%s: a model takes %d components at most", who, MDNS_SUM_MAX_COMPONENTS);
		return false;
	}
	if (m->ndim() + more > MDNS_MAX_DIM) { set_error("%s: %d parameters > %d", who, m->ndim() + more, MDNS_MAX_DIM); return false; }
	return true;
}

// a [nx] array of the caller's on the device, in a block of its own; `what` names it in the messages
static bool sum_array(const mdns_sum *m, const char *who, const char *what, const double *v, DeviceBuffer<double> *out)
{
	for (int j = 0; j < m->nx; j++)
		if (!std::isfinite(v[j])) { set_error("%s: %s[%d] = %g is not finite", who, what, j, v[j]); return false; }
	Context *c = ctx();
	if (!c) return false;
	DeviceBuffer<double> block;
	const size_t bytes = (size_t) m->nx * sizeof(double);
	if (!block.make((size_t) m->nx) || !MDNS_HIP(hipMemcpyAsync(block.get(), v, bytes, hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipStreamSynchronize(c->stream)))
		return false;                                                     // (the local owner frees what was made)
	*out = std::move(block);
	return true;
}

// the component is in: its place in the row, its flag
static void sum_append(mdns_sum *m, int kind, int nparams, int attenuated)
{
	const int k = m->ncomp++;
	m->kind[k] = kind;
	m->at[k] = m->nparams;
	m->attenuated[k] = attenuated ? 1 : 0;
	m->nparams += nparams;
}

extern "C" int mdns_sum_add_table(mdns_sum *m, int d, const int *n, const double *axes, int nw, const double *grid, const double *table,
                                  int flags, const double *ext, int attenuated)
{
	const char *who = "mdns_sum_add_table";
	const int known = MDNS_TABLE_REDSHIFT | MDNS_TABLE_AMPLITUDE | MDNS_TABLE_EXTINCTION | MDNS_TABLE_BROADEN;
	// (a d or flags that table_create refuses adds nothing here: that refusal is the message)
	int more = 0;
	if (d >= 1 && d <= MDNS_TABLE_MAX_AXES && !(flags & ~known)) {
		more = d;
		for (int bit = 1; bit <= MDNS_TABLE_BROADEN; bit <<= 1) more += (flags & bit) ? 1 : 0;
	}
	if (!sum_open(m, who, more, true)) return 1;
	mdns_table *t = table_create(who, known, m->x.data(), m->nx, d, n, axes, nw, grid, table, flags, ext);
	if (!t) return 1;
	m->table[m->ncomp] = t;
	sum_append(m, MDNS_SUM_TABLE, t->ndim, attenuated);
	return 0;
}

extern "C" int mdns_sum_add_powerlaw(mdns_sum *m, const double *lx, int attenuated)
{
	const char *who = "mdns_sum_add_powerlaw";
	if (!sum_open(m, who, 2, true)) return 1;
	if (!lx) { set_error("%s: null argument", who); return 1; }
	if (!sum_array(m, who, "lx", lx, &m->d_lx[m->ncomp])) return 1;
	sum_append(m, MDNS_SUM_POWERLAW, 2, attenuated);
	return 0;
}

extern "C" int mdns_sum_add_gauss(mdns_sum *m, int attenuated)
{
	if (!sum_open(m, "mdns_sum_add_gauss", 3, true)) return 1;
	sum_append(m, MDNS_SUM_GAUSS, 3, attenuated);
	return 0;
}

extern "C" int mdns_sum_set_attenuation(mdns_sum *m, const double *att)
{
	const char *who = "mdns_sum_set_attenuation";
	if (m && !m->used && m->has_att) { set_error("%s: the model has its attenuation already", who); return 1; }
	if (!sum_open(m, who, 1, false)) return 1;
	if (!att) { set_error("%s: null argument", who); return 1; }
	if (!sum_array(m, who, "att", att, &m->d_att)) return 1;
	m->has_att = 1;
	return 0;
}

// what both forms check first; 1: refused, 0: go on, -1: nothing to do
static int sum_batch_check(const mdns_sum *m, const void *params, int B, const void *out, int ldc, const char *who)
{
	if (!ctx()) return 1;
	if (!sum_ready(m, who)) return 1;
	if (B < 0 || ldc < m->nx) { set_error("%s: bad sizes B=%d ldc=%d (nx=%d)", who, B, ldc, m->nx); return 1; }
	if (B == 0) return -1;
	if (!params || !out) { set_error("%s: null argument", who); return 1; }
	return 0;
}

extern "C" int mdns_sum_curves_batch_dev(mdns_sum *m, const double *d_params, int B, double *d_out, int ldc)
{
	const int rc = sum_batch_check(m, d_params, B, d_out, ldc, "mdns_sum_curves_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_sum_curves(m, d_params, B, d_out, ldc) ? 0 : 1;
}

extern "C" int mdns_sum_curves_batch(mdns_sum *m, const double *params, int B, double *out)
{
	Context *c = ctx();
	const int rc = sum_batch_check(m, params, B, out, m ? m->nx : 0, "mdns_sum_curves_batch");
	if (rc != 0) return rc > 0;
	const size_t np = (size_t) B * m->ndim(), no = (size_t) B * m->nx;
	if (!m->d_params.fit(np) || !m->d_out.fit(no)) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(m->d_params.get(), params, np * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (!launch_sum_curves(m, m->d_params.get(), B, m->d_out.get(), m->nx)) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(out, m->d_out.get(), no * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
