// The instrument response on the device (mdns.h Part 13): model curves on n_in fine bins are folded onto the data's nx
// channels through a sparse, mostly banded matrix -- RMF x ARF of an X-ray instrument, the line-spread function of a
// spectrograph -- between the kernel that makes the curves (the caller's, or mdns_table.hip) and the kernels that score
// them (mdns_curves.hip, K2).  response_fold() is the one place that decides; no scoring kernel knows.
//
// Every value is the chain of single rounded fp64 operations that mdns.h Part 13 writes out; this file is compiled with
// -ffp-contract=off so that no multiply meets an add in an FMA, and the numpy statement
// (massivedatans_amd/response.py, Response.statement) reproduces the kernel bit for bit.  The kernel is a gather: the
// FMAs it gives up cost nothing, and the matrix cores, whose accumulation order is another, are not used.
//
// THE LAYOUT.  The caller's CSR by channel would make neighbouring lanes read vals and cols a row length apart.  At
// creation the matrix is re-laid on the host per group of 64 channels -- a wave --, entry l of the 64 rows contiguous
// (sliced ELL): a wave's load of entry l is 512 contiguous bytes of vals and 256 of cols.  A group is as wide as its
// longest row; every row keeps its own length and the padding behind it is never multiplied (l < len_j guards it, so a
// NaN bin cannot leak through a padded zero).  In a banded response neighbouring channels read neighbouring bins: the
// curve reads of a wave fall into one window of a candidate's row.
#include "mdns_internal.h"
#include <cmath>
#include <vector>

namespace mdns {

// what the kernel takes by value (scalar loads, no lane touches memory for it)
struct ResponseView {
	const int *len;
	const long long *slice;
	const double *vals;
	const int *cols;
	int nx;
};

static constexpr int kFoldBlock = 256;         // channels per workgroup, one per thread: four groups of the layout
static constexpr int kFoldCands = 4;           // candidates per thread (DESIGN section 4 has the resource report of 2, 4, 8)
static_assert(kFoldBlock % 64 == 0, "a wave is one group of the layout");

// grid (ceil(nx / kFoldBlock), ceil(B / NB)): thread t of workgroup (x, y) folds channel j = x kFoldBlock + t of the
// candidates y NB .. y NB + NB - 1.  vals[p] and cols[p] are loaded once and used for all NB, one accumulator each, every
// chain in the statement's order.  A candidate at or past B reads candidate B - 1 again and stores nothing: no test in
// the loop.  Nothing a value is made of depends on B, on the candidate's place in the batch, on ldc or on ldo.
template <int NB>
__global__ __launch_bounds__(kFoldBlock) void k_response_fold(const ResponseView rv, const double *__restrict__ curves, int ldc, int B,
                                                              double *__restrict__ out, int ldo)
{
	const int j = blockIdx.x * kFoldBlock + threadIdx.x;
	if (j >= rv.nx) return;
	const int b0 = blockIdx.y * NB;
	const double *__restrict__ row[NB];
#pragma unroll
	for (int k = 0; k < NB; k++) row[k] = curves + (size_t) (b0 + k < B ? b0 + k : B - 1) * ldc;
	const int len = rv.len[j];
	const size_t at = (size_t) rv.slice[j >> 6] + (size_t) (j & 63);
	const double *__restrict__ vals = rv.vals + at;
	const int *__restrict__ cols = rv.cols + at;
	double acc[NB];
#pragma unroll
	for (int k = 0; k < NB; k++) acc[k] = 0.0;
	for (int l = 0; l < len; l++) {
		const double v = vals[(size_t) l * 64];
		const int c = cols[(size_t) l * 64];
#pragma unroll
		for (int k = 0; k < NB; k++) acc[k] = acc[k] + v * row[k][c];
	}
#pragma unroll
	for (int k = 0; k < NB; k++)
		if (b0 + k < B) out[(size_t) (b0 + k) * ldo + j] = acc[k];
}

bool launch_response_fold(const mdns_response *r, const double *d_curves, int ldc, int B, double *d_out, int ldo)
{
	Context *c = ctx();
	if (!c) return false;
	if (B <= 0) return true;
	const ResponseView rv = {r->d_len.get(), r->d_slice.get(), r->d_vals.get(), r->d_cols.get(), r->nx};
	const int most = 65535 * kFoldCands;                                  // (the candidates are the grid's y)
	for (int lo = 0; lo < B; lo += most) {
		const int nb = B - lo < most ? B - lo : most;
		const dim3 grid((unsigned) ((r->nx + kFoldBlock - 1) / kFoldBlock), (unsigned) ((nb + kFoldCands - 1) / kFoldCands));
		hipLaunchKernelGGL(k_response_fold<kFoldCands>, grid, dim3(kFoldBlock), 0, c->stream, rv, d_curves + (size_t) lo * ldc, ldc, nb,
		                   d_out + (size_t) lo * ldo, ldo);
		if (!launched("k_response_fold")) return false;
	}
	return true;
}

bool response_fold(mdns_spectra *s, const double **d_curves, int *ldc, int B)
{
	if (!s->response || B <= 0) return true;
	// (a refused growth leaves the buffer empty and the handles as they were: the next call asks again)
	if (!s->d_folded.fit((size_t) B * s->nx)) return false;
	if (!launch_response_fold(s->response, *d_curves, *ldc, B, s->d_folded.get(), s->nx)) return false;
	*d_curves = s->d_folded.get();
	*ldc = s->nx;
	return true;
}

}  // namespace mdns

using namespace mdns;

// host block -> a resident device block of exactly n elements (n == 0: one element that nothing reads)
template <typename T> static bool resident(Context *c, DeviceBuffer<T> &d, const std::vector<T> &h)
{
	return d.make(h.size()) &&
	       (h.empty() || MDNS_HIP(hipMemcpyAsync(d.get(), h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream)));
}

extern "C" mdns_response *mdns_response_create(int nx, int n_in, const long long *rowptr, const int *cols, const double *vals)
{
	const char *who = "mdns_response_create";
	// every rule of the statement, on the host arrays, before the device is asked for anything
	if (nx < 1 || nx > MDNS_TABLE_MAX_NX) { set_error("%s: nx=%d: 1 to %d channels", who, nx, MDNS_TABLE_MAX_NX); return nullptr; }
	if (n_in < 1 || n_in > MDNS_TABLE_MAX_NX) { set_error("%s: n_in=%d: 1 to %d bins", who, n_in, MDNS_TABLE_MAX_NX); return nullptr; }
	if (!rowptr) { set_error("%s: null rowptr", who); return nullptr; }
	if (rowptr[0] != 0) { set_error("%s: rowptr[0] = %lld: must be 0", who, rowptr[0]); return nullptr; }
	for (int j = 0; j < nx; j++) {
		if (rowptr[j + 1] < rowptr[j]) {
			set_error("%s: rowptr[%d] = %lld < rowptr[%d] = %lld: rowptr must be non-decreasing", who, j + 1, rowptr[j + 1], j, rowptr[j]);
			return nullptr;
		}
		if (rowptr[j + 1] > MDNS_TABLE_MAX_ELEMS) {
			set_error("%s: rowptr[%d] = %lld: %lld entries at most", who, j + 1, rowptr[j + 1], (long long) MDNS_TABLE_MAX_ELEMS);
			return nullptr;
		}
	}
	const long long nnz = rowptr[nx];
	if (nnz > 0 && (!cols || !vals)) { set_error("%s: null %s", who, cols ? "vals" : "cols"); return nullptr; }
	for (int j = 0; j < nx; j++)
		for (long long p = rowptr[j]; p < rowptr[j + 1]; p++) {
			if (cols[p] < 0 || cols[p] >= n_in) { set_error("%s: cols[%lld] = %d outside [0, %d) (channel %d)", who, p, cols[p], n_in, j); return nullptr; }
			if (p > rowptr[j] && cols[p] <= cols[p - 1]) {
				set_error("%s: cols[%lld] = %d after %d: cols must be strictly increasing inside a row (channel %d)", who, p, cols[p], cols[p - 1], j);
				return nullptr;
			}
			if (!std::isfinite(vals[p])) { set_error("%s: vals[%lld] = %g is not finite (channel %d)", who, p, vals[p], j); return nullptr; }
		}
	// the layout of the file header: group g begins at slice[g] and is 64 lanes x its longest row
	const int groups = (nx + 63) / 64;
	std::vector<long long> slice((size_t) groups);
	std::vector<int> len((size_t) nx);
	long long total = 0;
	for (int g = 0; g < groups; g++) {
		long long width = 0;
		for (int j = 64 * g; j < nx && j < 64 * (g + 1); j++) {
			len[j] = (int) (rowptr[j + 1] - rowptr[j]);                   // (<= n_in: strictly increasing inside [0, n_in))
			if (len[j] > width) width = len[j];
		}
		slice[g] = total;
		total += 64 * width;                                              // (<= 2^14 groups x 2^6 x 2^20: no overflow)
		if (total > MDNS_TABLE_MAX_ELEMS) {
			set_error("%s: laid out per 64 channels the matrix takes more than %lld entries up to channel group %d (one long row among short ones?)",
			          who, (long long) MDNS_TABLE_MAX_ELEMS, g);
			return nullptr;
		}
	}
	std::vector<double> lvals((size_t) total, 0.0);
	std::vector<int> lcols((size_t) total, 0);
	for (int j = 0; j < nx; j++) {
		const size_t at = (size_t) slice[j >> 6] + (size_t) (j & 63);
		for (int l = 0; l < len[j]; l++) {
			lvals[at + (size_t) l * 64] = vals[rowptr[j] + l];
			lcols[at + (size_t) l * 64] = cols[rowptr[j] + l];
		}
	}
	Context *c = ctx();
	if (!c) return nullptr;
	mdns_response *r = new mdns_response();
	r->nx = nx; r->n_in = n_in; r->nnz = nnz;
	const bool ok = resident(c, r->d_len, len) && resident(c, r->d_slice, slice) && resident(c, r->d_vals, lvals) &&
	                resident(c, r->d_cols, lcols) && MDNS_HIP(hipStreamSynchronize(c->stream));
	if (!ok) { delete r; return nullptr; }                                // (the owners free what was made)
	return r;
}

extern "C" int mdns_response_destroy(mdns_response *r)
{
	if (!r) return 0;
	if (r->attached > 0) {
		set_error("mdns_response_destroy: the response is attached to %d spectra handle%s (mdns_spectra_set_response(s, NULL) first)",
		          r->attached, r->attached == 1 ? "" : "s");
		return 1;
	}
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	delete r;
	return 0;
}

extern "C" int mdns_response_nx(const mdns_response *r) { return r ? r->nx : -1; }
extern "C" int mdns_response_nin(const mdns_response *r) { return r ? r->n_in : -1; }

// what both forms check first; 1: refused, 0: go on, -1: nothing to do
static int fold_batch_check(const mdns_response *r, const void *curves, int ldc, int B, const void *out, int ldo, const char *who)
{
	if (!ctx()) return 1;
	if (!r) { set_error("%s: null response handle", who); return 1; }
	if (B < 0 || ldc < r->n_in || ldo < r->nx) {
		set_error("%s: bad sizes B=%d ldc=%d (n_in=%d) ldo=%d (nx=%d)", who, B, ldc, r->n_in, ldo, r->nx);
		return 1;
	}
	if (B == 0) return -1;
	if (!curves || !out) { set_error("%s: null argument", who); return 1; }
	return 0;
}

extern "C" int mdns_response_fold_batch_dev(mdns_response *r, const double *d_curves, int ldc, int B, double *d_out, int ldo)
{
	const int rc = fold_batch_check(r, d_curves, ldc, B, d_out, ldo, "mdns_response_fold_batch_dev");
	if (rc != 0) return rc > 0;
	return launch_response_fold(r, d_curves, ldc, B, d_out, ldo) ? 0 : 1;
}

extern "C" int mdns_response_fold_batch(mdns_response *r, const double *curves, int B, double *out)
{
	Context *c = ctx();
	const int rc = fold_batch_check(r, curves, r ? r->n_in : 0, B, out, r ? r->nx : 0, "mdns_response_fold_batch");
	if (rc != 0) return rc > 0;
	const size_t ni = (size_t) B * r->n_in, no = (size_t) B * r->nx;
	if (!r->d_in.fit(ni) || !r->d_out.fit(no)) return 1;
	// (pageable memory: the runtime stages it; the call ends in a synchronise)
	if (!MDNS_HIP(hipMemcpyAsync(r->d_in.get(), curves, ni * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (!launch_response_fold(r, r->d_in.get(), r->n_in, B, r->d_out.get(), r->nx)) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(out, r->d_out.get(), no * sizeof(double), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}

extern "C" int mdns_spectra_set_response(mdns_spectra *s, mdns_response *r)
{
	if (!s) { set_error("mdns_spectra_set_response: null spectra handle"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_response: a joint state exists on these spectra (set the response first)"); return 1; }
	if (r && r->nx != s->nx) {
		set_error("mdns_spectra_set_response: the response folds onto %d channels, the spectra have %d", r->nx, s->nx);
		return 1;
	}
	// (a fold of the old response may still be running: whoever destroys it afterwards waits for the stream)
	if (s->response) s->response->attached--;
	s->response = r;
	if (r) r->attached++;
	return 0;
}
