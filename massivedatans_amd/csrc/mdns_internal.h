// Internal declarations shared by the translation units of libmdns_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "mdns.h"

namespace mdns {

// ---- error handling ---------------------------------------------------------------------
void set_error(const char *fmt, ...);
bool hip_ok(hipError_t e, const char *what, const char *file, int line);
#define MDNS_HIP(call) ::mdns::hip_ok((call), #call, __FILE__, __LINE__)
// behind every kernel launch: false (and the error set) when the launch of `name` was refused
bool launched(const char *name);

// Busy polls of mapped mailboxes give up after MDNS_POLL_TIMEOUT_S seconds (default 120): a wedged
// kernel or a lost mailbox store becomes an error the caller can act on instead of a core spinning
// forever.
// wait_seq polls *at (mapped host memory a kernel on the context's stream raises last) until it holds `want`, looking
// at the stream now and then: a failed launch shows up as an error instead of a hang.  ok: everything the kernel
// stored before `want` can be read; timeout: the limit passed (the kernel may still be running); failed: the stream
// reports *err; empty: the stream drained and the number is not there.
enum class Wait { ok, timeout, failed, empty };
Wait wait_seq(const volatile unsigned long long *at, unsigned long long want, hipError_t *err = nullptr);
// What a wait that did not succeed becomes under the caller's name for what it waited for: "<who>: no result within
// MDNS_POLL_TIMEOUT_S", "<who> failed: <the stream's error>", "<who> finished without a result".  True: the number is
// there and no text was set.  (A caller that has something to put right after Wait::empty still holds the value.)
bool wait_ok(Wait w, hipError_t err, const char *who);

// ---- owned memory: grow-only scratch and exact-size blocks ------------------------------------
// Two owners, DeviceBuffer<T> and PinnedBuffer, and two ways to fill one:
//   fit(n)   grow-only SCRATCH of a call: holds >= n afterwards, made half as much again so that the next, slightly
//            larger call finds room; contents are not kept across a growth.
//   make(n)  a RESIDENT block of a handle (d_y, live, h_box ...): exactly n, at least one element, made once and kept
//            until the owner dies or is made again.  No growth policy: a resident array must not take half as much again.
// Handles hold owners, so `delete handle` (after ONE synchronise of the stream) frees everything and no destroy function
// lists members.  Everything else (kernel arguments, JointArrays, JointTrail, typed mailbox pointers, last_yT ...) is
// a view: a raw pointer taken with get() AFTER the owner is made.  A group of blocks made lazily on first use is made
// in locals or under all_or_none(), and its views are set last: it is whole or absent, never half there.
//
// How large a block that has to hold `need` elements of `elem` bytes is made by fit(): half as much again, in whole pages
// of 4 KiB.  The ONE growth policy of every DeviceBuffer and PinnedBuffer.
constexpr size_t grown_bytes(size_t need, size_t elem) { return ((need + need / 2) * elem + 4095) / 4096 * 4096; }
static_assert(grown_bytes(0, 8) == 0, "nothing asked, nothing made");
static_assert(grown_bytes(1, 8) == 4096, "one element: one page");
static_assert(grown_bytes(341, 8) == 4096, "341 + 170 doubles = 4088 bytes: still one page");
static_assert(grown_bytes(342, 8) == 8192, "342 + 171 doubles = 4104 bytes: two pages");
// and by make(): what is asked, one element at least
constexpr size_t exact_bytes(size_t need, size_t elem) { return (need ? need : 1) * elem; }
static_assert(exact_bytes(0, 8) == 8, "nothing asked: one element, as hipMalloc(0) hands out nothing to own");
static_assert(exact_bytes(342, 8) == 2736, "342 doubles are 342 doubles: no half again, no page rounding");
// The allocating path (mdns_core.hip): a block that exists is freed once the context's current stream has drained -- a
// kernel may still be using it --, a first allocation waits for nothing.  zero: the new block is cleared over all its
// `bytes`, in stream order; flags: as hipHostMalloc takes them.  nullptr (and the error set) on any failure; the old
// block is gone either way.
void *device_regrow(void *old, size_t bytes, bool zero);
void *pinned_regrow(void *old, size_t bytes, unsigned flags);
void scratch_free(void *p, bool host);
void *scratch_dev_pointer(void *host_block);       // of a mapped block; nullptr (and the error set) on failure

// An owning block of device memory for `cap()` elements.
template <typename T> class DeviceBuffer {
public:
	DeviceBuffer() = default;
	DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
	DeviceBuffer &operator=(DeviceBuffer &&o) noexcept
	{
		if (this != &o) { release(); p_ = o.p_; cap_ = o.cap_; o.p_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	~DeviceBuffer() { release(); }
	T *get() const { return p_; }
	size_t cap() const { return cap_; }
	// holds >= n elements afterwards; contents are NOT kept across a growth.  false (error set): the buffer is empty
	bool fit(size_t n) { return n <= cap_ || alloc(grown_bytes(n, sizeof(T)), false); }
	// the same; a newly allocated block is zero over its whole capacity, in stream order
	bool fit_zeroed(size_t n) { return n <= cap_ || alloc(grown_bytes(n, sizeof(T)), true); }
	// holds exactly max(n, 1) elements afterwards (zero: cleared in stream order), whatever it held before
	bool make(size_t n, bool zero = false) { return alloc(exact_bytes(n, sizeof(T)), zero); }
	// (whoever calls has made sure that nothing on the device uses the block any more)
	void release() { if (p_) scratch_free(p_, false); p_ = nullptr; cap_ = 0; }
private:
	bool alloc(size_t bytes, bool zero)
	{
		p_ = (T *) device_regrow(p_, bytes, zero);
		cap_ = p_ ? bytes / sizeof(T) : 0;
		return p_ != nullptr;
	}
	T *p_ = nullptr;
	size_t cap_ = 0;
};

// The same for pinned host memory, counted in bytes; `flags` as hipHostMalloc takes them (they travel with a move).
// dev(): a mapped block as the device sees it.
class PinnedBuffer {
public:
	explicit PinnedBuffer(unsigned flags = hipHostMallocDefault) : flags_(flags) {}
	PinnedBuffer(PinnedBuffer &&o) noexcept : p_(o.p_), dev_(o.dev_), cap_(o.cap_), flags_(o.flags_) { o.p_ = o.dev_ = nullptr; o.cap_ = 0; }
	PinnedBuffer &operator=(PinnedBuffer &&o) noexcept
	{
		if (this != &o) { release(); p_ = o.p_; dev_ = o.dev_; cap_ = o.cap_; flags_ = o.flags_; o.p_ = o.dev_ = nullptr; o.cap_ = 0; }
		return *this;
	}
	~PinnedBuffer() { release(); }
	char *get() const { return p_; }
	char *dev() const { return dev_; }
	size_t cap() const { return cap_; }
	bool fit(size_t bytes) { return bytes <= cap_ || alloc(grown_bytes(bytes, 1)); }
	// exactly max(bytes, 1) bytes, all zero, whatever it held before
	bool make(size_t bytes)
	{
		if (!alloc(exact_bytes(bytes, 1))) return false;
		memset(p_, 0, cap_);
		return true;
	}
	void release() { if (p_) scratch_free(p_, true); p_ = dev_ = nullptr; cap_ = 0; }
private:
	bool alloc(size_t want)
	{
		p_ = (char *) pinned_regrow(p_, want, flags_);
		dev_ = nullptr; cap_ = 0;
		if (p_ && (flags_ & hipHostMallocMapped) && !(dev_ = (char *) scratch_dev_pointer(p_))) release();
		if (p_) cap_ = want;
		return p_ != nullptr;
	}
	char *p_ = nullptr, *dev_ = nullptr;
	size_t cap_ = 0;
	unsigned flags_;
};

// A group of blocks that only make sense together: `ok` is the && chain that made (and cleared, and filled) them;
// when it failed every one of them is released, so the group is whole or absent and the next call tries again.
template <class... B> bool all_or_none(bool ok, B &...b)
{
	if (!ok) (b.release(), ...);
	return ok;
}

// ---- per-process context (one process drives one GPU) -----------------------------------
struct Context {
	int device = -1;
	hipStream_t own_stream = nullptr;
	hipStream_t stream = nullptr;     // stream every launch goes to (own_stream unless overridden)
	int num_cus = 256;
	// grow-only scratch of the process: device workspace, packed bootstrap masks, pinned host staging
	DeviceBuffer<char> d_ws, d_mask;
	PinnedBuffer h_pin;
	// staging of mdns_region_count_polled: pinned + mapped; its ticket (one int, zero between launches)
	PinnedBuffer count_stage{hipHostMallocMapped};
	DeviceBuffer<int> count_ticket;
	// partial sums of squares and tickets of launch_gauss_model_tsq's shared tiles (the tickets zero between launches)
	DeviceBuffer<double> tsq_part;
	DeviceBuffer<int> tsq_tickets;
	DeviceBuffer<unsigned> fold_tickets;       // of the folded K6 merge (mdns_neighbors.hip), zero between launches
	DeviceBuffer<double> mfma_zeros;           // 16 zeros for k_gauss_mfma_direct (mdns_chunk.hip)
	// stream-K form of the K2 matrix-core filter (mdns_k2gemm.hip): scratch tiles and delivery counts, zero whenever
	// no launch is in flight; tiled templates; 64 zeros
	DeviceBuffer<double> sk_scratch, sk_templ, sk_zeros;
	DeviceBuffer<unsigned> sk_delivered;
};
// nullptr (and mdns_last_error set) when no device can be initialised
Context *ctx();
// scratch accessors; return nullptr on allocation failure.  Contents are NOT preserved
// across a growing call.
void *device_scratch(size_t bytes);
void *pinned_scratch(size_t bytes);
void *mask_scratch(size_t bytes);      // packed bootstrap masks (separate from device_scratch)

// ---- resident spectra -------------------------------------------------------------------
// a caller-chosen emission-line list (mdns_spectra_set_lines): G rows (mu, a, sigma), line `ref` has its ratio fixed
// to 1.  Travels to k_lines_model BY VALUE (152 bytes of kernel arguments: the wave reads it with scalar loads,
// no lane touches memory for it).
static constexpr int kLinesMax = 6;
struct LineTable { double mu[kLinesMax], a[kLinesMax], sg[kLinesMax]; int ref; };
static constexpr int kJointParamsMost = kLinesMax + 2;     // parameters of a candidate at most (joint state staging)
}  // namespace mdns

struct mdns_spectra {
	int ndata = 0;      // number of spectra (rows)
	int nx = 0;         // channels per spectrum
	int ld = 0;         // row stride in doubles (nx rounded up to even => 16-byte aligned rows)
	// resident blocks, made once at their exact size (make); "or empty": get() == nullptr
	mdns::DeviceBuffer<double> d_y;    // [ndata, ld]   one spectrum per row
	mdns::DeviceBuffer<double> d_yT;   // [ldT/64][cols_nx(nx)][64] channel-major replica in tiles of 64 spectra
	                                   // (K1 lane kernel), or empty
	int ldT = 0;                       // ndata rounded up to a multiple of 64 (zero padded)
	mdns::DeviceBuffer<double> d_w;    // [ndata, ld] inverse variances 1/v (K2), or empty
	mdns::DeviceBuffer<double> d_x;    // [nx] wavelength grid, or empty
	mdns::DeviceBuffer<double> d_ysq;  // [ndata] sum of squares of every spectrum (K1 accept filter), or empty
	mdns::DeviceBuffer<double> d_yG;   // K1 on the matrix cores with operands straight from memory (k_gauss_gemm_filter): the spectra in
	                                   // tiles of 16 rows, channel pair by channel pair (tiled16_at), channels padded to 16; or empty
	mdns::DeviceBuffer<double> d_selG;                 // the same of the current selection
	mdns::DeviceBuffer<double> d_model_g;              // templates in the same tiling
	// per-handle grow-only device buffers for the host-pointer batch API
	mdns::DeviceBuffer<double> d_model;                // [B, ldm]
	mdns::DeviceBuffer<double> d_params;
	mdns::DeviceBuffer<int> d_rows;
	mdns::DeviceBuffer<double> d_out;
	mdns::DeviceBuffer<double> d_sel;                  // compact replica of the current selection (K1 lane kernel)
	// K2 on the matrix cores (mdns_k2gemm.hip), made on first use: y w and w [ndata, ldf] with ldf = nx rounded
	// up to 16 (zero padded), A = sum y^2 w [ndata]; all five or none (muse_filter_prepare)
	mdns::DeviceBuffer<double> d_fyw, d_fw, d_fa;
	mdns::DeviceBuffer<double> d_fyw_t, d_fw_t;         // the same two in tiles of 16 rows (mdns_k2gemm.hip, tiled_at)
	int ldf = 0;
	// the template model: nlines == 0 the built-in three lines (k_muse3_model, 5 parameters), else `lines`
	// (k_lines_model, nlines + 2 parameters); fixed once a joint state exists on the handle (njoint)
	int nlines = 0;
	mdns::LineTable lines = {};
	int njoint = 0;
	// per-spectrum polynomial continuum profiled out of the scale-marginalised likelihood (mdns_continuum.hip,
	// mdns_spectra_set_continuum): P = 0 off, else 1..4 Legendre terms in t; d_ct [model_ld(nx)] the channels mapped to
	// [-1, 1] (zero padded), d_cfac [ndata][kContRec] per spectrum the Cholesky factor of G = sum w b b^T (off-diagonal
	// entries, then the RECIPROCALS of the diagonal) and beta = G^-1 sum w b y.  Fixed like the line list (njoint)
	int continuum = 0;
	mdns::DeviceBuffer<double> d_ct, d_cfac;
	// fixed-scale chi^2 with the per-pixel weights d_w (mdns_curves.hip, mdns_spectra_set_fixed_scale): 1 = every curve
	// scoring of a joint state on this handle is -0.5 sum w (c - y)^2 and the state takes curve chunks only.  Needs
	// variances, excludes a continuum; fixed like the line list (njoint)
	int fixed_scale = 0;
	// photon counts (mdns_curves.hip, mdns_spectra_set_counts): 1 = d_y holds counts n, d_e [ndata, ld] the exposures
	// (0 = a masked pixel, whose n is 0 too; zero behind channel nx), d_koff [ndata] the host's offsets K; every curve
	// scoring of a joint state on this handle is the Poisson likelihood sum (n log c - e c) + K and the state takes curve
	// chunks only.  Excludes variances (d_w means 1/v to every K2 function); fixed like the line list (njoint)
	int counts = 0;
	mdns::DeviceBuffer<double> d_e, d_koff;
	// a background spectrum per count spectrum (mdns_curves.hip, mdns_spectra_set_background; needs counts): 1 = d_b
	// [ndata, ld] holds the background region's counts b, d_g its exposures g (area ratio included), d_kw [ndata] the
	// host's offsets Kw; a pixel masked on either side holds n = e = b = g = 0.  Every curve scoring of a joint state on
	// this handle is then the W statistic (k_curve_rows_b); fixed like the line list (njoint)
	int background = 0;
	mdns::DeviceBuffer<double> d_b, d_g, d_kw;
	// the instrument response (mdns_response.hip, mdns_spectra_set_response; mdns.h Part 13), borrowed, or nullptr: with
	// one every curve entry takes curves of response->n_in bins and response_fold() puts them, folded onto the nx
	// channels, into d_folded [B][nx] (grow-only) before anything scores them.  Fixed like the line list (njoint)
	mdns_response *response = nullptr;
	mdns::DeviceBuffer<double> d_folded;
};

// an instrument response on the device (mdns.h Part 13, mdns_response.hip): validated once at creation, never changed.
// The matrix per group of 64 channels (a wave), entry l of the 64 rows contiguous: entry l of channel j is element
// d_slice[j / 64] + 64 l + j % 64 of d_vals and d_cols, for l < d_len[j]; a group is as wide as its longest row and
// what lies behind a row's length is padding (vals 0, cols 0) that nothing multiplies
struct mdns_response {
	int nx = 0;         // output channels
	int n_in = 0;       // model bins
	long long nnz = 0;
	int attached = 0;   // spectra handles that borrow this response (mdns_spectra_set_response)
	// resident blocks, made once at their exact size
	mdns::DeviceBuffer<int> d_len;            // [nx]
	mdns::DeviceBuffer<long long> d_slice;    // [ceil(nx / 64)]
	mdns::DeviceBuffer<double> d_vals;        // the groups one after the other
	mdns::DeviceBuffer<int> d_cols;
	// grow-only scratch of the host-pointer batch call
	mdns::DeviceBuffer<double> d_in, d_out;
};

// a tabulated template grid on the device (mdns.h Part 12, mdns_table.hip): validated once at creation, never changed
struct mdns_table {
	int nx = 0;         // channels of the abscissa the curves are made on
	int d = 0;          // grid axes (1 .. MDNS_TABLE_MAX_AXES)
	int nw = 0;         // knots of the templates' own abscissa
	int ndim = 0;       // parameters per candidate: d [+ z] [+ E] [+ s] [+ A]
	int flags = 0;      // MDNS_TABLE_REDSHIFT | MDNS_TABLE_AMPLITUDE | MDNS_TABLE_EXTINCTION | MDNS_TABLE_BROADEN
	int n[MDNS_TABLE_MAX_AXES] = {};
	// resident blocks, made once at their exact size
	mdns::DeviceBuffer<double> d_x;       // [nx]
	mdns::DeviceBuffer<double> d_axes;    // the axes one after the other
	mdns::DeviceBuffer<double> d_grid;    // [nw]
	mdns::DeviceBuffer<double> d_table;   // [n_1] .. [n_d][nw]
	mdns::DeviceBuffer<double> d_ext;     // [nw] exponent per unit E (MDNS_TABLE_EXTINCTION), or empty
	mdns::DeviceBuffer<double> d_delta;   // [nw] quadrature widths of the knots (MDNS_TABLE_BROADEN), or empty
	// grow-only scratch of the host-pointer batch call
	mdns::DeviceBuffer<double> d_params, d_out;
	// grow-only scratch of the broadening route: the blended and the broadened templates [B][nw]
	mdns::DeviceBuffer<double> d_S, d_R;
};

// a sum of components as the model (mdns.h Part 14, mdns_sum.hip): built by the add entries, fixed at its first use
struct mdns_sum {
	int nx = 0;         // bins of the abscissa the curves are made on
	int ncomp = 0;      // components, in the order they were added
	int nparams = 0;    // parameters of the components together; a candidate's row has nparams + has_att
	int has_att = 0;    // 1: the common attenuation is set and N stands last in the row
	int used = 0;       // 1: a curves, init or draw call has run; nothing is added any more
	int kind[MDNS_SUM_MAX_COMPONENTS] = {};        // MDNS_SUM_TABLE | MDNS_SUM_POWERLAW | MDNS_SUM_GAUSS
	int at[MDNS_SUM_MAX_COMPONENTS] = {};          // where the component's parameters begin in a row
	int attenuated[MDNS_SUM_MAX_COMPONENTS] = {};
	mdns_table *table[MDNS_SUM_MAX_COMPONENTS] = {};           // OWNED: a TABLE component's table on this x, else nullptr
	mdns::DeviceBuffer<double> d_lx[MDNS_SUM_MAX_COMPONENTS];  // [nx] of a POWERLAW component, else empty
	std::vector<double> x;                 // the host's copy: what mdns_sum_add_table builds its table on
	// resident blocks, made once at their exact size
	mdns::DeviceBuffer<double> d_x;        // [nx]
	mdns::DeviceBuffer<double> d_att;      // [nx] the attenuation's exponent per unit N, or empty
	// grow-only scratch: the table components' curves [tables][B][nx]; the host-pointer batch call's two blocks
	mdns::DeviceBuffer<double> d_tcurves, d_params, d_out;
	int ndim() const { return nparams + has_att; }
};

namespace mdns {

// the table model's curves for d_params [B][t->ndim] -> d_out [B][ldc] (ldc >= t->nx; the padding is not touched),
// asynchronous on ctx()->stream (mdns_table.hip: k_table_curves, or the k_table_los_* route the handle's flags select,
// which may grow the handle's scratch)
bool launch_table_curves(mdns_table *t, const double *d_params, int B, double *d_out, int ldc);
// the same for candidates whose rows lie pstride >= t->ndim doubles apart (a slice of wider rows: mdns_sum.hip)
bool launch_table_curves(mdns_table *t, const double *d_params, int B, double *d_out, int ldc, int pstride);
// what every entry that makes a table goes through (mdns_table.hip): `who` names the entry in the messages, `known` the
// flag bits it takes.  All or none: nullptr (the error set) and nothing left allocated
mdns_table *table_create(const char *who, int known, const double *x, int nx, int d, const int *n, const double *axes, int nw,
                         const double *grid, const double *table, int flags, const double *ext);

// a sum model (mdns_sum.hip; mdns.h Part 14).  sum_ready: false (the error set under `who`) for a null handle or a model
// without components.  launch_sum_curves: d_params [B][m->ndim] -> d_out [B][ldc] (ldc >= m->nx; the padding is not
// touched), asynchronous on ctx()->stream: launch_table_curves per table component into the handle's grow-only scratch,
// then k_sum_curves.  The model is fixed from the first call on
bool sum_ready(const mdns_sum *m, const char *who);
bool launch_sum_curves(mdns_sum *m, const double *d_params, int B, double *d_out, int ldc);

// the instrument response (mdns_response.hip; mdns.h Part 13), asynchronous on ctx()->stream:
// d_curves [B][ldc] (ldc >= r->n_in) -> d_out [B][ldo] (ldo >= r->nx); the padding is neither read nor written
bool launch_response_fold(const mdns_response *r, const double *d_curves, int ldc, int B, double *d_out, int ldo);
// bins of a model curve for s: the response's n_in, or nx without one
inline int curve_bins(const mdns_spectra *s) { return s->response ? s->response->n_in : s->nx; }
// THE place that decides whether curves are folded: with a response on s, *d_curves [B][*ldc] is folded into
// s->d_folded [B][nx] and *d_curves, *ldc name that block afterwards; without one nothing happens.  false (the error
// set): the folded buffer could not grow, or the launch was refused
bool response_fold(mdns_spectra *s, const double **d_curves, int *ldc, int B);

// model row stride for nx channels: multiple of 512 doubles (zero padded), so that every
// lane / thread of the row kernels can load its channel pair without a bounds test
inline int model_ld(int nx) { return nx <= 0 ? 512 : ((nx + 511) / 512) * 512; }

// channel count of the channel-major replica / transposed templates: padded (with zeros) to
// the software-pipeline depth of k_gauss_cols
inline int cols_nx(int nx) { return ((nx + 7) / 8) * 8; }
// grow-only device buffers of a spectra handle (contents not kept): templates, compact replica
bool ensure_model(mdns_spectra *s, size_t doubles);
bool ensure_selection(mdns_spectra *s, size_t doubles);
// K1 through the lane kernel whatever the shape (mdns_core.hip)
int gauss_loglike_cols_dev(mdns_spectra *s, const double *d_params, int B, double noise_level,
                           const int *d_row_ids, int M, double *d_Lout);
// launchers implemented in mdns_like.hip (all asynchronous on ctx()->stream)
bool launch_gauss_model(const double *d_x, int nx, const double *d_params, int B,
                        double *d_model, int ldm);
// candidates per wave of k_gauss_cols for M selected spectra and B candidates (1..16)
int gauss_cols_tile(int M, int B);
// tiled templates MT[ceil(B/bt)][cols_nx(nx)][bt], zero for b >= B and j >= nx
// (d_zero, nzero): a small int buffer the kernel clears on the way (accept flags + result header)
bool launch_gauss_model_t(const double *d_x, int nx, const double *d_params, int B, int bt,
                          double *d_model_t, int *d_zero = nullptr, int nzero = 0);
// What k_joint_prepare saw of a data set's live column when it fixed the threshold, for the appends that follow
// (shelf_append): with it they need no second pass over the column.  It describes the column as it stood in epoch
// `epoch` of the state; every entry that writes live values starts a new epoch (joint_new_epoch, mdns_joint.hip), so a
// record never outlives the column it was read from.  Zeroed memory is no record: epochs start at 1.
struct alignas(32) JointRecord {
	double key;                    // the threshold prepare wrote to higher[d]
	double next;                   // the smallest live value > key, +inf if there is none
	unsigned long long epoch;      // JointArrays::epoch when it was written
	int cnt, pad;                  // live values <= key
};
// device arrays of the joint sampler state (mdns_joint.hip), all indexed by original data set
struct JointArrays {
	double *live;      // [nlive][ndata]   live-point likelihoods (multi_nested_sampler.py:111)
	double *shelfL;    // [cap][ndata]     likelihoods waiting on the shelves (:117)
	int *shelfn;       // [ndata]          how many
	double *higher;    // [ndata]          threshold of the next draw (:438-447)
	int nlive, cap, ndata;
	JointRecord *rec;  // [ndata]          prepare's view of the live column (a NaN live value: not counted, never `next`)
	unsigned long long epoch;              // the state's current epoch: a record of another one is not used
};
// what a chunk of a constrained draw leaves for the host (mdns.h, mdns_joint_commit_dev)
struct JointHeader { int accepted; int status; long long pad; };
// What the accept pass leaves behind for the candidates it flags: per (candidate, tile of 64
// selected spectra) in which some lane beat its threshold, the ballot word and the 64
// likelihoods -- all a commit needs when nobody asks for the whole likelihood row.  Entries are
// valid when their stamp is the current one (nothing is ever cleared).
struct JointTrail {
	int *stamp_of;                 // [candidates x tiles]      (nullptr: no trail)
	unsigned long long *word;      // [candidates x tiles]
	double *L;                     // [candidates x tiles][64]
	int stamp;
};
// What a commit leaves for a caller that does not want the likelihood row, in host memory
// mapped into the device: the host polls `seq` instead of copying and synchronising.
struct JointMailbox { unsigned long long seq; int accepted; int status; unsigned long long bits[1]; /* ceil(M/64) words */ };
// a draw chunk in two launches (mdns_chunk.hip): whether the shape qualifies, and the launchers.
// Candidates (and, for the first chunk of a draw, the selection's row ids) are read from host
// memory mapped into the device; accepted candidates get flags[b] = stamp.
bool chunk_fits(const mdns_spectra *s, int M, int B);
bool launch_chunk_accept(const mdns_spectra *s, const double *d_params_mapped, int B, double scale,
                         const int *d_rows_in, int *d_rows_dev, int M, const double *d_higher,
                         int *d_flags, int stamp, const JointTrail &trail, void *d_header);
bool launch_chunk_commit(const int *d_thr_rows, int M, int B, const int *d_flags, int stamp, const JointTrail &trail,
                         const JointArrays &st, void *d_header, unsigned long long *d_fillbits, void *box_dev,
                         unsigned long long seq);
// accept test fused into the lane kernel: flags[b] = 1 when candidate b beats a threshold
bool launch_gauss_cols_accept(const mdns_spectra *s, const double *d_yT, const double *d_model_t, int bt, int B,
                              double scale, const int *d_rows, const int *d_thr_rows, int M,
                              const double *d_higher, int *d_flags, const JointTrail &trail);
// the accept test as guarded filter (mdns_like.hip, k_gauss_cols_filter): same flags and trail as
// launch_gauss_cols_accept
// 0: the chain kernel decides; 1: vector-FMA filter; 2: matrix-core filter
int gauss_filter_pays(const mdns_spectra *s, int M, int B);
int gauss_filter_tile(int M, int B);
// d_model_g != nullptr (bt = 16): the templates also in the tiled16 layout
bool launch_gauss_model_tsq(const double *d_x, int nx, const double *d_params, int B, int bt, double *d_model_t, double *d_msq,
                            int *d_zero, int nzero, double *d_model_g = nullptr);
bool launch_gauss_cols_filter(const mdns_spectra *s, const double *d_yT, const double *d_model_t, int bt, int B,
                              double scale, const int *d_rows, const int *d_thr_rows, int M,
                              const double *d_higher, int *d_flags, const double *d_msq, const JointTrail &trail, int *d_lowest);
bool launch_row_sumsq(const double *d_y, int ld, int nx, int ndata, double *d_out);
// element (row r, channel c) of an operand in tiles of 16 rows, inside a tile channel pair by channel pair, 16 rows x 2
// doubles: the 16 lanes of a quarter wave (the same channels of 16 rows) read 256 contiguous bytes; ncp = channels / 2
#ifdef __HIPCC__
__host__ __device__
#endif
inline size_t tiled16_at(size_t r, int c, int ncp) { return (((r >> 4) * (size_t) ncp + (size_t) (c >> 1)) << 5) + ((r & 15) << 1) + (size_t) (c & 1); }
inline int tiled16_nx(int nx) { return (nx + 15) & ~15; }
// rows [M or ndata][ld] (d_rows: which, or nullptr) -> tiled16 replica, zero padded
bool launch_tile_rows16(const double *d_y, int ld, int M, int nx, const int *d_rows, double *d_out);
// the same decision on the matrix cores (mdns_chunk.hip, k_gauss_mfma_filter + k_exact_list);
// templates tiled 16 wide; d_scratch int32[MDNS_JOINT_MAX_BATCH + 16], zeroed once
bool launch_gauss_mfma_filter(const mdns_spectra *s, const double *d_yT, const double *d_model_t, int B, double scale,
                              const int *d_thr_rows, int M, const double *d_higher, int *d_flags,
                              const double *d_msq, const JointTrail &trail, int *d_lowest, int *d_scratch, void *d_header,
                              const double *d_yG = nullptr, const double *d_model_g = nullptr);
// which form of the matrix-core filter: 0 staged through LDS (round 3), 1 operands straight from memory in the layouts
// of the lane kernel (opt-in), 2 operands straight from memory, tiled16 (needs d_yG / d_model_g)
int gauss_mfma_form();
// first flagged candidate from the trail of the accept pass: fill bits, shelf appends, thresholds
// (flag_value: what the accept pass wrote into d_flags for an accepted candidate)
// box_dev != nullptr: the kernel's last workgroup also fills the mailbox (no k_joint_publish behind it); d_ticket: an int, zero
// between launches
bool launch_joint_commit_trail(const int *d_thr_rows, int M, int B, const int *d_flags, const JointTrail &trail,
                               const JointArrays &st, void *d_header, unsigned long long *d_fillbits, int flag_value = 1,
                               void *box_dev = nullptr, unsigned long long seq = 0, int *d_ticket = nullptr);
// first flagged candidate: its likelihood row, fill bits, shelf appends, new thresholds
bool launch_gauss_cols_commit(const mdns_spectra *s, const double *d_yT, const double *d_model_t, int mstride, int B,
                              double scale, const int *d_rows, const int *d_thr_rows, int M, const int *d_flags,
                              const JointArrays &st, void *d_header, unsigned long long *d_fillbits, double *d_Lrow);
bool launch_gauss_cols(const mdns_spectra *s, const double *d_yT, const double *d_model_t, int bt, int B,
                       double scale, const int *d_rows, int M, double *d_out);
// templates of the handle's model for d_params [B][muse_nparams(s)] -> d_model [B][ldm], zero padded: the built-in
// three lines (k_muse3_model) or the handle's line list (k_lines_model<G>)
inline int muse_nparams(const mdns_spectra *s) { return s->nlines ? s->nlines + 2 : 5; }
bool launch_muse_model(const mdns_spectra *s, const double *d_params, int B, double *d_model, int ldm);
bool launch_gauss_rows(const mdns_spectra *s, const double *d_model, int ldm, int B,
                       double scale, const int *d_rows, int M, double *d_out);
struct MuseBandFused;
// the most channels the k_muse_rows<NP, .> / k_muse_rows2<NP> instantiations take (NP <= 8); longer spectra go to
// k_muse_rows_generic
static constexpr int kMuseRowsNxMost = 4096;
// band != nullptr (pairs of candidates only: muse_rows_variant(...) == 1, and nx <= kMuseRowsNxMost: the generic kernel
// carries no vote -- refused, never dropped): the band test of the likelihood noise and its mailbox ride along with
// the scoring -- no k_joint_band behind it
bool launch_muse_rows(const mdns_spectra *s, const double *d_model, int ldm, int B,
                      const int *d_rows, int M, double *d_out, int B_shape = 0, const MuseBandFused *band = nullptr);
int muse_rows_variant(int B, int M);
// the same likelihood with the handle's polynomial continuum profiled out per spectrum (mdns_continuum.hip; what
// launch_muse_rows launches when s->continuum > 0).  d_scale [B][M] and d_coef [B][M][P] (either may be nullptr): the
// fitted scale and continuum coefficients of every pair
static constexpr int kContMax = 4;             // terms at most
static constexpr int kContRec = 16;            // doubles per spectrum in d_cfac: 6 off-diagonal, 4 reciprocal diagonal, 4 beta, 2 unused
bool launch_continuum_rows(const mdns_spectra *s, const double *d_model, int ldm, int B, const int *d_rows, int M,
                           double *d_out, double *d_scale, double *d_coef);
// the band test of a chunk (mdns_joint.hip, k_joint_band) on K2 as two matrix products (mdns_k2gemm.hip):
// where its outcome goes (device memory; clear / maybe per candidate, listed pairs behind a counter)
struct MuseBandOut { int *counter, *clear, *maybe, *pair_b, *pair_k; double *pair_L, *pair_thr; int cap; int *zero_at; };
bool muse_filter_applies(const mdns_spectra *s, int B, int M);
int muse_filter_ld(int nx);              // row stride of its operands; templates of a chunk it may take: model_ld(nx) + 16 apart
bool launch_muse_filter(mdns_spectra *s, const double *d_model, int ldm, int B, const int *d_rows, int M,
                        const double *d_higher, const double *d_bound, const MuseBandOut &out);
void muse_filter_note(int which);          // 1: a chunk scored again exactly, 2: an exact row for a commit
// src [nx][lds] -> dst [ndata][ld] (only the nx x ndata corner is touched)
bool launch_transpose(const double *d_src, int nx, int ndata, double *d_dst, int ld,
                      bool invert, int lds);
// rows [ndata][ld] -> tiled channel-major replica [ceil(ndata/64)][cols_nx(nx)][64]
bool launch_tile_columns(const double *d_y, int ld, int ndata, int nx, const int *d_rows, double *d_yt);
bool launch_copy_rows(const double *d_src, int nx, int ndata, double *d_dst, int ld,
                      bool invert);
bool launch_pad_model(const double *d_src, int nx, int B, double *d_dst, int ldm);
// caller-made model curves (mdns_curves.hip): d_curves [B][ldc] against the selected rows of s, d_out [B][M], one chain
// per pair with the channels ascending.  The statistic:
//   kCurveNoise    -0.5 sum_j ((c_j - y_j) / noise_level)^2                                       (k_curve_rows)
//   kCurveChi2     -0.5 sum_j w_j (c_j - y_j)^2 with the per-pixel weights s->d_w, which must be there (k_curve_rows_w)
//   kCurvePoisson  sum_j (n_j log max(c_j, DBL_MIN) - e_j c_j) + K of a handle in counts mode: s->d_e, s->d_koff must be
//                  there                                                (k_curve_log into s->d_model, then k_curve_rows_p)
//   kCurveWstat    the W statistic's -W/2 of a handle with a background (s->d_b, s->d_g, s->d_kw must be there), the
//                  background rate of every pixel profiled out                                    (k_curve_rows_b)
//   kCurveMarginal no curve kernel: spectra with variances whose scale is marginalised (launch_curve_pad, then K2)
// curve_stat: what every curve scoring of a joint state on the handle is (fixed_scale, counts, background: mdns_spectra)
enum CurveStat { kCurveNoise, kCurveChi2, kCurvePoisson, kCurveWstat, kCurveMarginal };
CurveStat curve_stat(const mdns_spectra *s);
bool launch_curve(CurveStat stat, mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                  const int *d_rows, int M, double *d_out);
// the curves as the K2 row kernels take templates, [B][ldm] zero padded
bool launch_curve_pad(const double *d_curves, int ldc, int nx, int B, double *d_model, int ldm);
// d_out [B][M][nx] = the W statistic's profiled rate itself (k_curve_background, the device functions of k_curve_rows_b)
bool launch_curve_background(const mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_rows, int M, double *d_out);

// launchers implemented in mdns_neighbors.hip
// What a radius computation leaves behind: written by the LAST workgroup of the bootstrap
// kernel to finish (it alone knows that all per-round maxima are final), once into device
// memory for the membership kernel that follows in stream order and once into mapped host
// memory, where the host finds it by polling `seq` -- no event, no copy, no second stream.
struct RegionResult {
	double radius;                 // sqrt(max_b round_sq[b])            cneighbors.c:160-174
	double thresh;                 // smallest T with sqrt(T) >= radius  cneighbors.c:88,109
	unsigned long long seq;        // written last
	unsigned long long pad;
};
struct BootstrapFinish {
	unsigned *counter;             // device; zero outside a launch
	RegionResult *d_res;           // device copy
	RegionResult *h_res;           // mapped, host-coherent copy
	unsigned long long seq;        // the value `seq` takes for this computation
};

// threshold on the squared distance: thresh_sq, or -- when d_res != nullptr -- the one the
// preceding radius computation left on the device
// mdns_region_create_bootstrapped without the wait for the radius (mdns_core.hip)
mdns_region *region_begin_bootstrapped(const double *members, int K, int ndim, const unsigned *packed, int nbootstraps);

// mail != nullptr: `d_cands` and `d_counts` may be host memory mapped into the device -- the kernel
// reads the candidates from there, stores the counts there (no member split) and its last
// workgroup raises *seq_at to `seq`: the host polls instead of copying both ways
struct CountMail { int *ticket; unsigned long long *seq_at; unsigned long long seq; };
bool launch_count_within(const double *d_members, int K, int ndim, double thresh_sq,
                         const RegionResult *d_res, const double *d_cands, int M, int *d_counts,
                         const CountMail *mail = nullptr);
bool launch_bootstrap(const double *d_members, int K, int ndim, const double *d_chosen,
                      int nbootstraps, double *d_round_sq, const BootstrapFinish *finish = nullptr);
// the same with the choice already packed: bit b of d_packed[i] = point i is chosen in round b
bool launch_bootstrap_packed(const double *d_members, int K, int ndim, const unsigned *d_packed,
                             int nbootstraps, double *d_round_sq, const BootstrapFinish *finish);
bool launch_nn_maxsq(const double *d_members, int K, int ndim, double *d_out);
// K6 with the pool in Morton order and tile culling (mdns_k6sort.hip): the same radius, bit for bit
bool bootstrap_sorted_applies(int K, int ndim, int nbootstraps);
bool launch_bootstrap_sorted(const double *d_members, int K, int ndim, const unsigned *d_packed, int nbootstraps,
                             double *d_round_sq, const BootstrapFinish *finish);

// ---- the first batch of a region without a host look in between (mdns_chain.hip) --------
// what the chain kernels need of a region whose radius computation has been launched (mdns_core.hip)
struct RegionView { const double *d_members; int K, ndim; const RegionResult *d_res; };
bool region_view(mdns_region *r, RegionView *out);
static constexpr int kChainMost = 1024;        // proposals per batch at most (radfriendsregion.py:124 uses 1000)
static constexpr int kChainDim = 8;            // dimensions at most
// by-value description of what happens to a proposal between the membership test and the kernel:
// the metric's inverse transform (sdml.py), the unit-cube test (hiermetriclearn.py:113-116), the prior
// transform and the kernel's parameters (mdns_prior)
struct ChainSpec {
	int n, ndim, nparams, limit, identity;
	double mn[kChainDim], mx[kChainDim];                   // extent of the members (radfriendsregion.py:69-70)
	double mean[kChainDim], scale[kChainDim];              // y * scale + mean
	double a[kChainDim], b[kChainDim];
	int pow10[kChainDim], kernel_pow10[kChainDim];
};
// mapped host memory the chain kernels fill: {seq | nkept, B | counts | parameters of the candidates scored}
struct ChainBox {
	unsigned long long seq;
	int nkept, B;
	int counts[kChainMost];
	double params[kChainMost][3];
	double u[kChainMost * kChainDim];                      // in: the raw doubles of the proposals
};
// proposals lo + (hi - lo) u from the raw doubles in `box_dev->u`, radius and threshold from d_res;
// counts to box_dev->counts and d_counts, proposals to d_props [n][ndim]; mail != nullptr: the last
// workgroup raises box->seq (a chain that ends here)
bool launch_box_count(const RegionView &rv, const ChainSpec &spec, ChainBox *box_dev, double *d_props, int *d_counts,
                      const CountMail *mail);
// k_chunk_accept with the candidates taken from the kept proposals (first min(kept, limit) of them)
bool launch_chain_accept(const mdns_spectra *s, const ChainSpec &spec, const double *d_props, const int *d_counts,
                         ChainBox *box_dev, double scale, const int *d_rows_in, int *d_rows_dev, int M,
                         const double *d_higher, int *d_flags, int stamp, const JointTrail &trail, void *d_header);

// optional per-launch event timing (mdns_profile); which: 0 gauss rows, 1 muse rows,
// 2 count-within, 3 nearest-chosen.  Use as:  { ProfileScope ps(which); launch...; }
struct ProfileScope {
	int slot;
	explicit ProfileScope(int which);
	~ProfileScope();
};
// name of the kernel instantiation last launched for class `which` (mdns_profile_kernel)
void note_kernel(int which, const char *fmt, ...);

// Between workgroups of ONE launch: what one hands to another goes through agent-scope atomic stores / loads (or
// atomics) -- they act on memory itself -- and the hand-over is an agent-scope atomic ticket; all the fence has to
// do is wait for this wave's outstanding memory operations.  __threadfence() also writes back and invalidates the
// XCD's whole L2, per workgroup that calls it (measured in round 4: a launch of 256 workgroups with two such
// fences each took 365 us instead of 176; the folded K6 merge 264 us instead of 51).
#ifdef __HIPCC__
// (the workgroup-scope fence orders the compiler's view and emits no instruction; the wait is what makes the stores
// and atomics of THIS wave complete -- acknowledged by memory -- before the ticket that follows: on gfx9 vmcnt counts
// them too.  An agent-scope release fence is exactly `buffer_wbl2 sc1` + this wait.)
__device__ __forceinline__ void handover_release()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
__device__ __forceinline__ void handover_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); }
// Into host memory mapped into the device, for a host that polls `seq`: system-scope stores act on that memory
// itself, so `seq` only has to wait for the stores before it (every thread: mail_store()s, handover_release(), a
// barrier; then one thread: mail_raise()).  A system-scope RELEASE would write back the L2 first -- per mailbox
// a few microseconds that nobody needs: what the host reads is all in the mailbox.
template <class T, class V> __device__ __forceinline__ void mail_store(T *at, V v) { __hip_atomic_store(at, (T) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
__device__ __forceinline__ void mail_raise(unsigned long long *seq_at, unsigned long long seq) { handover_release(); mail_store(seq_at, seq); }

// Sum over the 64 lanes of a wavefront, returned in every lane (wave-uniform).
// Data-parallel primitives (DPP) move the partial sums inside the VALU -- no LDS crossbar
// round trips as with ds_bpermute shuffles, which made reductions the longest part of the row
// kernels.  Steps: the two quad permutations, row_shr:4, row_shr:8 (each 16-lane row now has its
// sum in lanes 12-15), row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3; lane 63
// holds the total.  Lanes without a source receive 0 (bound_ctrl), the identity of the sum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double v)
{
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, true);
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, true);
	return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double wave_sum(double v)
{
	v += dpp_move<0xb1, 0xf>(v);      // quad_perm:[1,0,3,2]
	v += dpp_move<0x4e, 0xf>(v);      // quad_perm:[2,3,0,1]
	v += dpp_move<0x114, 0xf>(v);     // row_shr:4
	v += dpp_move<0x118, 0xf>(v);     // row_shr:8
	v += dpp_move<0x142, 0xa>(v);     // row_bcast:15 -> rows 1, 3
	v += dpp_move<0x143, 0xc>(v);     // row_bcast:31 -> rows 2, 3
	const int lo = __builtin_amdgcn_readlane(__double2loint(v), 63);
	const int hi = __builtin_amdgcn_readlane(__double2hiint(v), 63);
	return __hiloint2double(hi, lo);
}

// ---- what the commit kernels share (mdns_like.hip, mdns_chunk.hip, mdns_joint.hip) ----
// Likelihood L, which beats the threshold `thr` of data set d, goes onto d's shelf, and d gets its next threshold
// (multi_nested_sampler.py:482-485, :438-447; the numpy statement is HostJointState.commit / _threshold in
// jointstate.py).  With n waiting the threshold was the (n+1)-th smallest of live + shelf, and L lies above it: the
// (n+2)-th smallest of the enlarged set is the old threshold again when it occurs more than once, else the smaller of
// L and the next value above it.  False, and nothing changed, when the shelf is full: the caller raises its status
// bit.  One lane per data set: no two callers share state.
// The live part of the two questions -- how many values at or below thr, which is the next one above -- is answered by
// prepare's record when that is of this epoch and for this very threshold (a first append since prepare, or a later one
// after appends that left the threshold where it was): then only the n shelf entries are walked.  Otherwise (the
// threshold has moved, or there is no record) the column is scanned, U live-point loads in flight at a time (the latency
// of a round trip, not the count, is what this pass costs).  Counts and fmin do not depend on the order, so the result
// depends neither on U nor on which of the two answered.
template <int U>
__device__ __forceinline__ bool shelf_append(const JointArrays &st, int d, double L, double thr)
{
	// shelfn[d], the record and the caller's higher[d] leave together: nothing branches on one of them before all are
	// asked for (the full shelf is refused below, in front of the stores: with a branch up here the compiler moves the
	// other loads behind it)
	const int n = st.shelfn[d];
	const JointRecord rec = st.rec[d];
	int at_most = 0;
	double next = INFINITY;
	if (rec.epoch == st.epoch && rec.key == thr) {
		at_most = rec.cnt;
		next = rec.next;
	} else {
		int p = 0;
		for (; p + U <= st.nlive; p += U) {
			double v[U];
#pragma unroll
			for (int u = 0; u < U; u++) v[u] = st.live[(size_t) (p + u) * st.ndata + d];
#pragma unroll
			for (int u = 0; u < U; u++) { if (v[u] <= thr) at_most++; else next = fmin(next, v[u]); }
		}
		for (; p < st.nlive; p++) {
			const double v = st.live[(size_t) p * st.ndata + d];
			if (v <= thr) at_most++; else next = fmin(next, v);
		}
	}
	for (int e = 0; e < n; e++) {
		const double v = st.shelfL[(size_t) e * st.ndata + d];
		if (v <= thr) at_most++; else next = fmin(next, v);
	}
	if (n >= st.cap) return false;
	st.shelfL[(size_t) n * st.ndata + d] = L;
	st.shelfn[d] = n + 1;
	st.higher[d] = at_most >= n + 2 ? thr : fmin(L, next);
	return true;
}

// The first flagged candidate is THE accepted point (hiermetriclearn.py:193-196): the lowest b < B with
// flagged(flags[b]), or INT_MAX.  Every thread of the workgroup (BLOCK threads) calls; s_first: an LDS int of the
// caller's.
template <int BLOCK, class Flagged>
__device__ __forceinline__ int first_flagged(int *s_first, const int *__restrict__ flags, int B, Flagged flagged)
{
	if (threadIdx.x == 0) *s_first = 0x7fffffff;
	__syncthreads();
	for (int b = threadIdx.x; b < B; b += BLOCK)
		if (flagged(flags[b])) { atomicMin(s_first, b); break; }      // ascending per thread: its first is its lowest
	__syncthreads();
	return *s_first;
}

// Accept test of a wave of the lane kernels (lane = spectrum `lane` of tile `tile`, all lanes on candidate `cand`):
// when some lane beats its threshold (thr NaN: a lane past the selection, never) and cand < B, the candidate is flagged
// and the trail keeps the ballot word and the 64 likelihoods.  Returns the word.
__device__ __forceinline__ unsigned long long trail_vote(const JointTrail &trail, int *__restrict__ flags, int cand, int B,
                                                         int ntiles, int tile, int lane, double L, double thr)
{
	const unsigned long long word = __ballot(L > thr);
	if (word != 0ull && cand < B) {                                    // rare: a candidate some data set accepts
		const size_t at = (size_t) cand * ntiles + tile;
		if (trail.stamp_of) trail.L[at * 64 + lane] = L;
		if (lane == 0) {
			flags[cand] = 1;
			if (trail.stamp_of) { trail.word[at] = word; trail.stamp_of[at] = trail.stamp; }
		}
	}
	return word;
}
#endif


// ---- the likelihood noise in band form (mdns.h: draw_band / draw_band_commit; kernels in mdns_joint.hip, mdns_like.hip) ----
// every likelihood against its threshold +- (1.01 bound[b] + 1e-12 (|L| + |thr|)): a pair above the band is beaten whatever
// the noise (clear[b] = 1), a pair inside it is listed for the host, which alone makes the exact deviates
#ifdef __HIPCC__
static constexpr int kBandCap = 4096;
struct BandBox {                   // mapped host memory
	unsigned long long seq;
	int npairs, pad;
	int status[MDNS_JOINT_MAX_BATCH];
	int pair_b[kBandCap], pair_k[kBandCap];
	double pair_L[kBandCap], pair_thr[kBandCap];
};
struct BandScratch {               // device memory
	int counter, ticket;           // listed pairs; workgroups of the band pass that are done (zero between launches)
	int clear[MDNS_JOINT_MAX_BATCH], maybe[MDNS_JOINT_MAX_BATCH];
	int pair_b[kBandCap], pair_k[kBandCap];
	double pair_L[kBandCap], pair_thr[kBandCap];
};

// what the host needs of a band pass, into mapped memory (`seq` last), and the scratch ready for the next chunk:
// by one workgroup that knows every vote is in (a kernel of its own behind the pass, or the pass's last workgroup)
__device__ __forceinline__ void band_publish(BandScratch *__restrict__ sc, int B, BandBox *__restrict__ box, unsigned long long seq)
{
	const int n = __hip_atomic_load(&sc->counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	const int m = n < kBandCap ? n : kBandCap;
	for (int b = threadIdx.x; b < B; b += (int) blockDim.x) {
		const int cl = __hip_atomic_load(&sc->clear[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const int mb = __hip_atomic_load(&sc->maybe[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		mail_store(&box->status[b], cl ? 1 : (mb ? 2 : 0));
		sc->clear[b] = 0; sc->maybe[b] = 0;
	}
	for (int t = threadIdx.x; t < m; t += (int) blockDim.x) {
		mail_store(&box->pair_b[t], __hip_atomic_load(&sc->pair_b[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		mail_store(&box->pair_k[t], __hip_atomic_load(&sc->pair_k[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		mail_store(&box->pair_L[t], __hip_atomic_load(&sc->pair_L[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
		mail_store(&box->pair_thr[t], __hip_atomic_load(&sc->pair_thr[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
	}
	handover_release();
	__syncthreads();
	if (threadIdx.x != 0) return;
	sc->counter = 0;
	sc->ticket = 0;
	mail_store(&box->npairs, n);
	mail_raise(&box->seq, seq);
}

// one (candidate, data set) pair of a band pass (votes and pairs through agent-scope stores: whoever publishes may be
// another workgroup of the same launch)
__device__ __forceinline__ void band_vote(BandScratch *__restrict__ sc, int b, int k, double v, double thr, double bnd)
{
	const double band = 1.01 * bnd + 1e-12 * (fabs(v) + fabs(thr));
	if (v > thr + band) __hip_atomic_store(&sc->clear[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	else if (v >= thr - band) {
		__hip_atomic_store(&sc->maybe[b], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		const int at = atomicAdd(&sc->counter, 1);
		if (at < kBandCap) {
			__hip_atomic_store(&sc->pair_b[at], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(&sc->pair_k[at], k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(&sc->pair_L[at], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			__hip_atomic_store(&sc->pair_thr[at], thr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		}
	}
}
// a scoring kernel that votes and publishes by itself (launch_muse_rows): sc == nullptr: it does neither
struct MuseBandFused { BandScratch *sc; BandBox *box; unsigned long long seq; const double *higher; const double *bound; int *status_zero; };
#endif

// smallest double T with sqrt(T) >= r, so that  sqrt(d) < r  <=>  d < T  for every d >= 0
double sqrt_threshold(double r);

}  // namespace mdns
