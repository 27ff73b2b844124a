// libmdns_hip.so -- context, memory, resident spectra and the host-pointer entry points.
// Kernels live in mdns_like.hip and mdns_neighbors.hip.
#include "mdns_internal.h"
#include <time.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace mdns {

// ---------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------
static char g_error[512] = "";

void set_error(const char *fmt, ...)
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(g_error, sizeof(g_error), fmt, ap);
	va_end(ap);
	if (getenv("MDNS_VERBOSE")) fprintf(stderr, "[mdns] %s\n", g_error);
}

bool hip_ok(hipError_t e, const char *what, const char *file, int line)
{
	if (e == hipSuccess) return true;
	set_error("%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
	return false;
}

bool launched(const char *name)
{
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) return true;
	set_error("launch of %s failed: %s", name, hipGetErrorString(e));
	return false;
}

// ---------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------
// never destroyed: its buffers must not be freed through a runtime that is torn down at exit
static Context &g_ctx = *new Context;
static bool g_ctx_ready = false;
static std::mutex g_ctx_mutex;

static int init_locked(int device)
{
	if (g_ctx_ready && (device < 0 || device == g_ctx.device)) return 0;
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
		set_error("no HIP device visible: libmdns_hip has no CPU path");
		return 1;
	}
	if (device < 0) {
		const char *e = getenv("MDNS_DEVICE");
		if (e && *e) device = atoi(e);
		else if ((e = getenv("LOCAL_RANK")) && *e) device = atoi(e) % count;
		else device = 0;
	}
	if (device >= count) {
		set_error("device %d requested but only %d visible", device, count);
		return 1;
	}
	if (g_ctx_ready) {
		// One process drives ONE GPU (include/mdns.h): spectra, regions, result slots, pooled
		// buffers and events all live on the first device; handing them to another one would use
		// them across devices.
		set_error("mdns_init(%d): this process already runs on device %d; one process drives one GPU "
		          "(start one process per GPU)", device, g_ctx.device);
		return 1;
	}
	if (!MDNS_HIP(hipSetDevice(device))) return 1;
	hipDeviceProp_t prop;
	if (!MDNS_HIP(hipGetDeviceProperties(&prop, device))) return 1;
	g_ctx.device = device;
	g_ctx.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
	if (!MDNS_HIP(hipStreamCreateWithFlags(&g_ctx.own_stream, hipStreamNonBlocking))) return 1;
	g_ctx.stream = g_ctx.own_stream;
	g_ctx_ready = true;
	return 0;
}

Context *ctx()
{
	std::lock_guard<std::mutex> lock(g_ctx_mutex);
	if (!g_ctx_ready && init_locked(-1) != 0) return nullptr;
	// the runtime's current device is per thread: make sure it is ours
	(void) hipSetDevice(g_ctx.device);
	return &g_ctx;
}

void *device_scratch(size_t bytes) { Context *c = ctx(); return c && c->d_ws.fit(bytes) ? c->d_ws.get() : nullptr; }
void *mask_scratch(size_t bytes) { Context *c = ctx(); return c && c->d_mask.fit(bytes) ? c->d_mask.get() : nullptr; }
void *pinned_scratch(size_t bytes) { Context *c = ctx(); return c && c->h_pin.fit(bytes) ? c->h_pin.get() : nullptr; }

void scratch_free(void *p, bool host) { (void) (host ? hipHostFree(p) : hipFree(p)); }

// a block that exists may still be in use by a kernel on the stream: wait, then free it.  nullptr: no context
static Context *drop_old(void *old, bool host)
{
	Context *c = ctx();
	if (old) { if (c) (void) hipStreamSynchronize(c->stream); scratch_free(old, host); }
	return c;
}

void *device_regrow(void *old, size_t bytes, bool zero)
{
	Context *c = drop_old(old, false);
	void *p = nullptr;
	if (!c || !MDNS_HIP(hipMalloc(&p, bytes))) return nullptr;
	if (zero && !MDNS_HIP(hipMemsetAsync(p, 0, bytes, c->stream))) { (void) hipFree(p); return nullptr; }
	return p;
}

void *pinned_regrow(void *old, size_t bytes, unsigned flags)
{
	void *p = nullptr;
	return drop_old(old, true) && MDNS_HIP(hipHostMalloc(&p, bytes, flags)) ? p : nullptr;
}

void *scratch_dev_pointer(void *host_block)
{
	void *d = nullptr;
	return MDNS_HIP(hipHostGetDevicePointer(&d, host_block, 0)) ? d : nullptr;
}

// smallest non-negative double T with sqrt(T) >= r.  sqrt on doubles is correctly rounded
// and monotone, so  sqrt(d) < r  <=>  d < T.  Binary search over the bit patterns of the
// non-negative doubles (their integer order is their numeric order).
double sqrt_threshold(double r)
{
	if (std::isnan(r)) return r;             // d < NaN is false, as sqrt(d) < NaN is
	if (!(r > 0)) return 0.0;                // sqrt(d) >= 0 >= r: never inside
	if (std::isinf(r)) return r;             // every finite d is inside
	uint64_t lo = 0, hi;                     // predicate false at lo (sqrt(0) = 0 < r)
	double inf = INFINITY;
	memcpy(&hi, &inf, 8);                    // predicate true at +inf
	while (hi - lo > 1) {
		uint64_t mid = lo + (hi - lo) / 2;
		double t;
		memcpy(&t, &mid, 8);
		if (std::sqrt(t) >= r) hi = mid; else lo = mid;
	}
	double T;
	memcpy(&T, &hi, 8);
	return T;
}

// ---------------------------------------------------------------------------------------
// per-launch event timing
// ---------------------------------------------------------------------------------------
struct TimedLaunch { int which; hipEvent_t start, stop; };
static long long g_prof_seen[4];
static int g_prof_every = 1;
static int g_profiling = 0;                   // bit k: time launches of kernel class k
static std::vector<TimedLaunch> g_pending;
static std::vector<hipEvent_t> g_event_pool;
static long long g_prof_count[4] = {0, 0, 0, 0};
static double g_prof_ms[4] = {0, 0, 0, 0};

static hipEvent_t pooled_event()
{
	if (!g_event_pool.empty()) { hipEvent_t e = g_event_pool.back(); g_event_pool.pop_back(); return e; }
	hipEvent_t e = nullptr;
	if (hipEventCreate(&e) != hipSuccess) return nullptr;
	return e;
}

static void drain_pending()
{
	for (TimedLaunch &t : g_pending) {
		float ms = 0;
		if (hipEventSynchronize(t.stop) == hipSuccess && hipEventElapsedTime(&ms, t.start, t.stop) == hipSuccess) {
			g_prof_count[t.which] += 1;
			g_prof_ms[t.which] += ms;
		}
		g_event_pool.push_back(t.start);
		g_event_pool.push_back(t.stop);
	}
	g_pending.clear();
}

ProfileScope::ProfileScope(int which) : slot(-1)
{
	if (!(g_profiling & (1 << which)) || !g_ctx_ready) return;
	if (g_prof_seen[which]++ % g_prof_every != 0) return;      // sampled: every n-th launch of a class
	TimedLaunch t{which, pooled_event(), pooled_event()};
	if (!t.start || !t.stop) return;
	(void) hipEventRecord(t.start, g_ctx.stream);
	g_pending.push_back(t);
	slot = (int) g_pending.size() - 1;
}

ProfileScope::~ProfileScope()
{
	if (slot < 0) return;
	(void) hipEventRecord(g_pending[slot].stop, g_ctx.stream);
	if (g_pending.size() >= 4096) drain_pending();      // bound the number of live events
}

}  // namespace mdns

using namespace mdns;

// ---------------------------------------------------------------------------------------
// library state
// ---------------------------------------------------------------------------------------
extern "C" int mdns_abi_version(void) { return 1; }
extern "C" const char *mdns_last_error(void) { return g_error; }

extern "C" int mdns_device_count(void)
{
	int count = 0;
	if (hipGetDeviceCount(&count) != hipSuccess) return 0;
	return count;
}

extern "C" int mdns_init(int device)
{
	std::lock_guard<std::mutex> lock(g_ctx_mutex);
	return init_locked(device);
}

// ---------------------------------------------------------------------------------------
// raw device helpers
// ---------------------------------------------------------------------------------------
extern "C" void *mdns_dev_alloc(size_t bytes)
{
	if (!ctx()) return nullptr;
	void *p = nullptr;
	if (!MDNS_HIP(hipMalloc(&p, bytes ? bytes : 8))) return nullptr;
	return p;
}
extern "C" void mdns_dev_free(void *p) { if (p && ctx()) (void) hipFree(p); }
extern "C" int mdns_h2d(void *dst, const void *src, size_t bytes)
{
	Context *c = ctx();
	if (!c) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
extern "C" int mdns_d2h(void *dst, const void *src, size_t bytes)
{
	Context *c = ctx();
	if (!c) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
extern "C" int mdns_d2d(void *dst, const void *src, size_t bytes)
{
	Context *c = ctx();
	if (!c) return 1;
	return MDNS_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream)) ? 0 : 1;
}
extern "C" int mdns_sync(void)
{
	Context *c = ctx();
	if (!c) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
extern "C" int mdns_set_stream(void *hip_stream)
{
	Context *c = ctx();
	if (!c) return 1;
	c->stream = hip_stream ? (hipStream_t) hip_stream : c->own_stream;
	return 0;
}
extern "C" void *mdns_get_stream(void)
{
	Context *c = ctx();
	return c ? (void *) c->stream : nullptr;
}
extern "C" void *mdns_event_create(void)
{
	if (!ctx()) return nullptr;
	hipEvent_t ev;
	if (!MDNS_HIP(hipEventCreate(&ev))) return nullptr;
	return (void *) ev;
}
extern "C" void mdns_event_destroy(void *ev) { if (ev) (void) hipEventDestroy((hipEvent_t) ev); }
extern "C" int mdns_event_record(void *ev)
{
	Context *c = ctx();
	if (!c || !ev) return 1;
	return MDNS_HIP(hipEventRecord((hipEvent_t) ev, c->stream)) ? 0 : 1;
}
extern "C" double mdns_event_elapsed_ms(void *a, void *b)
{
	if (!a || !b) return NAN;
	if (!MDNS_HIP(hipEventSynchronize((hipEvent_t) b))) return NAN;
	float ms = 0;
	if (!MDNS_HIP(hipEventElapsedTime(&ms, (hipEvent_t) a, (hipEvent_t) b))) return NAN;
	return (double) ms;
}

extern "C" int mdns_profile(int classes)
{
	if (!ctx()) return 1;
	drain_pending();
	for (int k = 0; k < 4; k++)
		if (classes & (1 << k)) { g_prof_count[k] = 0; g_prof_ms[k] = 0; g_prof_seen[k] = 0; }
	g_profiling = classes & 15;
	return 0;
}
extern "C" int mdns_profile_every(int n)
{
	g_prof_every = n > 1 ? n : 1;
	return 0;
}
// Launchers call note_kernel on every launch (the region kernels among them, on the sampler step's critical path), so
// it only keeps the format and its arguments -- fmt is a literal with at most four %d (int) / %s (a literal) -- and
// mdns_profile_kernel puts the name together when somebody asks for it.
static constexpr int kNoteArgs = 4;
struct KernelNote { const char *fmt; int narg; int num[kNoteArgs]; const char *str[kNoteArgs]; };
static KernelNote g_kernel_note[4];
static char g_kernel_name[4][64];
void mdns::note_kernel(int which, const char *fmt, ...)
{
	if (which < 0 || which > 3) return;
	KernelNote &n = g_kernel_note[which];
	n.fmt = fmt;
	n.narg = 0;
	va_list ap;
	va_start(ap, fmt);
	for (const char *p = fmt; *p && n.narg < kNoteArgs; p++) {
		if (*p != '%') continue;
		if (!*++p) break;
		if (*p == 'd') { n.str[n.narg] = nullptr; n.num[n.narg++] = va_arg(ap, int); }
		else if (*p == 's') { n.num[n.narg] = 0; n.str[n.narg++] = va_arg(ap, const char *); }
	}
	va_end(ap);
}
extern "C" const char *mdns_profile_kernel(int which)
{
	if (which < 0 || which > 3) return "";
	const KernelNote &n = g_kernel_note[which];
	char *out = g_kernel_name[which];
	const size_t cap = sizeof g_kernel_name[which];
	size_t len = 0;
	int a = 0;
	out[0] = 0;
	for (const char *p = n.fmt; p && *p && len + 1 < cap; p++) {
		if (*p == '%' && (p[1] == 'd' || p[1] == 's') && a < n.narg) {
			const int w = n.str[a] ? snprintf(out + len, cap - len, "%s", n.str[a]) : snprintf(out + len, cap - len, "%d", n.num[a]);
			len = w < 0 || len + (size_t) w >= cap ? cap - 1 : len + (size_t) w;
			a++;
			p++;
		} else {
			out[len++] = *p;
			out[len] = 0;
		}
	}
	return out;
}
extern "C" int mdns_profile_read(int which, long long *launches, double *total_ms)
{
	if (!ctx() || which < 0 || which > 3) return 1;
	drain_pending();
	if (launches) *launches = g_prof_count[which];
	if (total_ms) *total_ms = g_prof_ms[which];
	return 0;
}

// ---------------------------------------------------------------------------------------
// resident spectra
// ---------------------------------------------------------------------------------------
static bool upload_rows(const double *h_src, int ndata, int nx, int layout, double *d_dst, int ld,
                        bool invert)
{
	// stage the host array as it is, then re-lay it on the device into [ndata, ld] rows
	Context *c = ctx();
	const size_t n = (size_t) ndata * nx;
	DeviceBuffer<double> tmp;
	if (!tmp.make(n)) return false;
	double *const d_tmp = tmp.get();
	bool ok = MDNS_HIP(hipMemcpyAsync(d_tmp, h_src, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
	if (ok) {
		if (layout == MDNS_LAYOUT_CHANNEL_MAJOR) ok = launch_transpose(d_tmp, nx, ndata, d_dst, ld, invert, ndata);
		else ok = launch_copy_rows(d_tmp, nx, ndata, d_dst, ld, invert);
	}
	return MDNS_HIP(hipStreamSynchronize(c->stream)) && ok;      // (drained before `tmp` goes)
}

extern "C" mdns_spectra *mdns_spectra_create(const double *x, const double *y, const double *v,
                                             int ndata, int nx, int layout)
{
	Context *c = ctx();
	if (!c) return nullptr;
	if (ndata < 0 || nx < 0 || !y || (layout != 0 && layout != 1)) {
		set_error("mdns_spectra_create: bad arguments (ndata=%d nx=%d layout=%d)", ndata, nx, layout);
		return nullptr;
	}
	mdns_spectra *s = new mdns_spectra();
	s->ndata = ndata; s->nx = nx; s->ld = (nx + 1) & ~1;
	// +2 doubles of slack: the row kernels read whole 16-byte pairs
	const size_t elems = (size_t) ndata * s->ld + 2;
	bool ok = s->d_y.make(elems, true);
	ok = ok && upload_rows(y, ndata, nx, layout, s->d_y.get(), s->ld, false);
	if (ok && !v && nx > 0 && ndata > 0) {
		// K1 also keeps a channel-major replica, in tiles of 64 spectra, for candidate batches
		// (the tiling kernel writes every element, padding included)
		s->ldT = ((ndata + 63) / 64) * 64;
		const size_t telems = (size_t) cols_nx(nx) * s->ldT;
		ok = s->d_yT.make(telems);
		ok = ok && launch_tile_columns(s->d_y.get(), s->ld, ndata, nx, nullptr, s->d_yT.get());
		ok = ok && s->d_ysq.make((size_t) ndata);
		ok = ok && launch_row_sumsq(s->d_y.get(), s->ld, nx, ndata, s->d_ysq.get());
		ok = ok && MDNS_HIP(hipStreamSynchronize(c->stream));
	}
	if (ok && v) {
		ok = s->d_w.make(elems, true);
		ok = ok && upload_rows(v, ndata, nx, layout, s->d_w.get(), s->ld, true);
	}
	if (ok && x) {
		ok = s->d_x.make((size_t) nx);
		ok = ok && MDNS_HIP(hipMemcpyAsync(s->d_x.get(), x, nx * sizeof(double), hipMemcpyHostToDevice, c->stream));
		ok = ok && MDNS_HIP(hipStreamSynchronize(c->stream));
	}
	if (!ok) { mdns_spectra_destroy(s); return nullptr; }
	return s;
}

extern "C" void mdns_spectra_destroy(mdns_spectra *s)
{
	if (!s) return;
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	if (s->response) s->response->attached--;                     // (borrowed: mdns.h Part 13)
	delete s;           // (its blocks free themselves)
}
extern "C" int mdns_spectra_ndata(const mdns_spectra *s) { return s ? s->ndata : -1; }
extern "C" int mdns_spectra_nparams(const mdns_spectra *s) { return s ? muse_nparams(s) : -1; }

extern "C" int mdns_spectra_set_lines(mdns_spectra *s, const double *lines, int G, int ref)
{
	if (!s) { set_error("mdns_spectra_set_lines: null spectra handle"); return 1; }
	if (s->njoint > 0) { set_error("mdns_spectra_set_lines: a joint state exists on these spectra (set the line list first)"); return 1; }
	if (G == 0) { s->nlines = 0; return 0; }
	if (G < 1 || G > kLinesMax || !lines) { set_error("mdns_spectra_set_lines: %d lines (1..%d)", G, kLinesMax); return 1; }
	if (ref < 0 || ref >= G) { set_error("mdns_spectra_set_lines: ref=%d outside [0,%d)", ref, G); return 1; }
	LineTable t = {};
	for (int g = 0; g < G; g++) {
		const double mu = lines[3 * g], a = lines[3 * g + 1], sg = lines[3 * g + 2];
		if (!std::isfinite(mu) || !std::isfinite(a) || !std::isfinite(sg) || !(sg > 0)) {
			set_error("mdns_spectra_set_lines: line %d = (%g, %g, %g): finite values and sigma > 0 are needed", g, mu, a, sg);
			return 1;
		}
		t.mu[g] = mu; t.a[g] = a; t.sg[g] = sg;
	}
	for (int g = G; g < kLinesMax; g++) t.sg[g] = 1.0;
	t.ref = ref;
	Context *c = ctx();
	if (c) (void) hipStreamSynchronize(c->stream);
	s->lines = t;
	s->nlines = G;
	return 0;
}
extern "C" int mdns_spectra_nx(const mdns_spectra *s) { return s ? s->nx : -1; }

// ---------------------------------------------------------------------------------------
// batched scoring, device pointers
// ---------------------------------------------------------------------------------------
static bool check_batch(const mdns_spectra *s, int B, int M, const char *who)
{
	if (!s) { set_error("%s: null spectra handle", who); return false; }
	if (B < 0 || M < 0 || M > s->ndata) {
		set_error("%s: bad sizes B=%d M=%d (ndata=%d)", who, B, M, s->ndata);
		return false;
	}
	return true;
}

namespace mdns {
bool ensure_model(mdns_spectra *s, size_t doubles) { return s->d_model.fit(doubles); }
bool ensure_selection(mdns_spectra *s, size_t doubles) { return s->d_sel.fit(doubles); }

// K1 with the lane kernel whatever the shape (one lane per spectrum, channels summed in
// ascending order): L[B, M] to d_Lout.  The likelihood of a (candidate, spectrum) pair computed
// here does not depend on B, M or the tile shape.
int gauss_loglike_cols_dev(mdns_spectra *s, const double *d_params, int B, double noise_level,
                           const int *d_row_ids, int M, double *d_Lout)
{
	if (!s->d_yT.get()) { set_error("the lane kernel needs the channel-major replica (spectra without variances)"); return 1; }
	const double scale = -0.5 / (noise_level * noise_level);
	const int bt = gauss_cols_tile(M, B);
	if (!ensure_model(s, (size_t) cols_nx(s->nx) * (B + bt))) return 1;
	if (!launch_gauss_model_t(s->d_x.get(), s->nx, d_params, B, bt, s->d_model.get())) return 1;
	// A selection is first copied into a compact replica (coalesced row reads, one pass)
	// when the lane kernel would otherwise gather its columns once per candidate tile:
	// many tiles, or a sparse selection (measured: 1 000 of 10 000 spectra, B = 256: 59 us
	// gathering in the kernel).
	const bool sparse = (size_t) M * 8 < (size_t) s->ndata;
	if (d_row_ids && (B >= 128 || sparse)) {
		if (!ensure_selection(s, (size_t) ((M + 63) / 64) * 64 * cols_nx(s->nx))) return 1;
		if (!launch_tile_columns(s->d_y.get(), s->ld, M, s->nx, d_row_ids, s->d_sel.get())) return 1;
		return launch_gauss_cols(s, s->d_sel.get(), s->d_model.get(), bt, B, scale, nullptr, M, d_Lout) ? 0 : 1;
	}
	return launch_gauss_cols(s, s->d_yT.get(), s->d_model.get(), bt, B, scale, d_row_ids, M, d_Lout) ? 0 : 1;
}
}  // namespace mdns

extern "C" int mdns_gauss_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                            double noise_level, const int *d_row_ids, int M,
                                            double *d_Lout)
{
	if (!ctx() || !check_batch(s, B, M, "mdns_gauss_loglike_batch_dev")) return 1;
	if (!s->d_x.get()) { set_error("spectra were created without a wavelength grid"); return 1; }
	if (B == 0 || M == 0) return 0;
	const double scale = -0.5 / (noise_level * noise_level);
	// Two kernels, chosen by shape only (never by data), so a run is reproducible:
	//  * batches of 12+ candidates on dense selections (at least one spectrum in eight), and
	//    batches of 32+ on any selection, are arithmetic-bound: one LANE per spectrum on the
	//    channel-major replica, templates as scalar operands (k_gauss_cols);
	//  * few candidates, or sparse selections, are bandwidth/latency-bound: one WAVE per
	//    spectrum row, reading exactly the selected rows once (k_gauss_rows).
	// Measured on MI355X, 10 000 x 200, all spectra: rows 6.8 / 8.7 / 12.3 / 18.9 us at
	// B = 1 / 4 / 8 / 16, cols 16.9 / 17.3 / 19.2 us at B = 8 / 16 / 32; at 10 % of the spectra
	// and B = 1024: cols 59 us, rows 688 us.
	static const char *forced = getenv("MDNS_K1_PATH");      // "rows" | "cols": experiments only
	const bool dense = (size_t) M * 8 >= (size_t) s->ndata;
	// dense: the lane kernel pays a ~17 us pipeline fill, the row kernel ~6.5 us plus more per
	// eval; they cross near 1.5e5 evals (B = 12 at 10 000 spectra, B = 2 at 100 000: 27 vs 38 us)
	bool use_cols = s->d_yT.get() && ((dense && B >= 2 && (long long) M * B >= 150000) || B >= 32);
	if (forced && !strcmp(forced, "rows")) use_cols = false;
	if (forced && !strcmp(forced, "cols") && s->d_yT.get()) use_cols = true;
	if (use_cols) return gauss_loglike_cols_dev(s, d_params, B, noise_level, d_row_ids, M, d_Lout);
	const int ldm = model_ld(s->nx);
	if (!s->d_model.fit((size_t) B * ldm)) return 1;
	if (!launch_gauss_model(s->d_x.get(), s->nx, d_params, B, s->d_model.get(), ldm)) return 1;
	return launch_gauss_rows(s, s->d_model.get(), ldm, B, scale, d_row_ids, M, d_Lout) ? 0 : 1;
}

extern "C" int mdns_muse_loglike_batch_dev(mdns_spectra *s, const double *d_ypred, int B,
                                           const int *d_row_ids, int M, double *d_Lout)
{
	if (!ctx() || !check_batch(s, B, M, "mdns_muse_loglike_batch_dev")) return 1;
	if (!s->d_w.get()) { set_error("spectra were created without variances"); return 1; }
	if (B == 0 || M == 0) return 0;
	int ldc = curve_bins(s);                                              // (rows of n_in bins with a response: folded to rows of nx)
	if (!response_fold(s, &d_ypred, &ldc, B)) return 1;
	const int ldm = model_ld(s->nx);
	if (!s->d_model.fit((size_t) B * ldm)) return 1;
	if (!launch_pad_model(d_ypred, s->nx, B, s->d_model.get(), ldm)) return 1;
	return launch_muse_rows(s, s->d_model.get(), ldm, B, d_row_ids, M, d_Lout) ? 0 : 1;
}

// templates of the handle's model (the built-in three lines or its line list), then K2
static int lines_loglike_dev(mdns_spectra *s, const double *d_params, int B, const int *d_row_ids, int M, double *d_Lout, const char *who)
{
	if (!ctx() || !check_batch(s, B, M, who)) return 1;
	if (!s->d_w.get() || !s->d_x.get()) { set_error("spectra need variances and a wavelength grid"); return 1; }
	if (B == 0 || M == 0) return 0;
	const int ldm = model_ld(s->nx);
	if (!s->d_model.fit((size_t) B * ldm)) return 1;
	if (!launch_muse_model(s, d_params, B, s->d_model.get(), ldm)) return 1;
	return launch_muse_rows(s, s->d_model.get(), ldm, B, d_row_ids, M, d_Lout) ? 0 : 1;
}

extern "C" int mdns_muse3_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                            const int *d_row_ids, int M, double *d_Lout)
{
	if (s && s->nlines) { set_error("mdns_muse3_loglike_batch_dev: a line list is set on these spectra (mdns_lines_loglike_batch_dev)"); return 1; }
	return lines_loglike_dev(s, d_params, B, d_row_ids, M, d_Lout, "mdns_muse3_loglike_batch_dev");
}

extern "C" int mdns_lines_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                            const int *d_row_ids, int M, double *d_Lout)
{
	return lines_loglike_dev(s, d_params, B, d_row_ids, M, d_Lout, "mdns_lines_loglike_batch_dev");
}

// ---------------------------------------------------------------------------------------
// batched scoring, host pointers
// ---------------------------------------------------------------------------------------
typedef int (*dev_batch_fn)(mdns_spectra *, const double *, int, const int *, int, double *, double);

static int host_batch(mdns_spectra *s, const double *params, int B, int nparam,
                      const int *row_ids, int M, double *Lout, double extra, dev_batch_fn fn,
                      const char *who)
{
	Context *c = ctx();
	if (!c || !check_batch(s, B, M, who)) return 1;
	if (B == 0 || M == 0) return 0;
	if (row_ids) {
		for (int k = 0; k < M; k++)
			if (row_ids[k] < 0 || row_ids[k] >= s->ndata) {
				set_error("%s: row_ids[%d]=%d outside [0,%d)", who, k, row_ids[k], s->ndata);
				return 1;
			}
	}
	const size_t np = (size_t) B * nparam, no = (size_t) B * M;
	if (!s->d_params.fit(np)) return 1;
	if (!s->d_out.fit(no)) return 1;
	if (row_ids && !s->d_rows.fit((size_t) M)) return 1;
	// stage through pinned memory so both copies are truly asynchronous
	const size_t stage_bytes = np * 8 + (row_ids ? (size_t) M * 4 : 0);
	const size_t out_off = (stage_bytes + 15) & ~(size_t) 15;
	char *pin = (char *) pinned_scratch(out_off + no * 8);
	if (!pin) return 1;
	memcpy(pin, params, np * 8);
	bool ok = MDNS_HIP(hipMemcpyAsync(s->d_params.get(), pin, np * 8, hipMemcpyHostToDevice, c->stream));
	if (ok && row_ids) {
		memcpy(pin + np * 8, row_ids, (size_t) M * 4);
		ok = MDNS_HIP(hipMemcpyAsync(s->d_rows.get(), pin + np * 8, (size_t) M * 4, hipMemcpyHostToDevice, c->stream));
	}
	if (!ok) return 1;
	if (fn(s, s->d_params.get(), B, row_ids ? s->d_rows.get() : nullptr, M, s->d_out.get(), extra) != 0) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(pin + out_off, s->d_out.get(), no * 8, hipMemcpyDeviceToHost, c->stream))) return 1;
	if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
	memcpy(Lout, pin + out_off, no * 8);
	return 0;
}

static int fn_gauss(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double noise)
{ return mdns_gauss_loglike_batch_dev(s, p, B, noise, r, M, o); }
static int fn_muse(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_muse_loglike_batch_dev(s, p, B, r, M, o); }
static int fn_muse3(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_muse3_loglike_batch_dev(s, p, B, r, M, o); }
static int fn_curve(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double noise)
{ return mdns_curve_loglike_batch_dev(s, p, curve_bins(s), B, noise, r, M, o); }
static int fn_curve_chi2(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_curve_chi2_batch_dev(s, p, curve_bins(s), B, r, M, o); }
static int fn_curve_poisson(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_curve_poisson_batch_dev(s, p, curve_bins(s), B, r, M, o); }
static int fn_curve_wstat(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_curve_wstat_batch_dev(s, p, curve_bins(s), B, r, M, o); }
static int fn_lines(mdns_spectra *s, const double *p, int B, const int *r, int M, double *o, double)
{ return mdns_lines_loglike_batch_dev(s, p, B, r, M, o); }

extern "C" int mdns_gauss_loglike_batch(mdns_spectra *s, const double *params, int B,
                                        double noise_level, const int *row_ids, int M, double *Lout)
{
	return host_batch(s, params, B, 3, row_ids, M, Lout, noise_level, fn_gauss, "mdns_gauss_loglike_batch");
}
extern "C" int mdns_curve_loglike_batch(mdns_spectra *s, const double *curves, int B, double noise_level,
                                        const int *row_ids, int M, double *Lout)
{
	return host_batch(s, curves, B, s ? curve_bins(s) : 0, row_ids, M, Lout, noise_level, fn_curve, "mdns_curve_loglike_batch");
}
extern "C" int mdns_curve_chi2_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout)
{
	return host_batch(s, curves, B, s ? curve_bins(s) : 0, row_ids, M, Lout, 0, fn_curve_chi2, "mdns_curve_chi2_batch");
}
extern "C" int mdns_curve_poisson_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout)
{
	return host_batch(s, curves, B, s ? curve_bins(s) : 0, row_ids, M, Lout, 0, fn_curve_poisson, "mdns_curve_poisson_batch");
}
extern "C" int mdns_curve_wstat_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout)
{
	return host_batch(s, curves, B, s ? curve_bins(s) : 0, row_ids, M, Lout, 0, fn_curve_wstat, "mdns_curve_wstat_batch");
}
extern "C" int mdns_muse_loglike_batch(mdns_spectra *s, const double *ypred, int B,
                                       const int *row_ids, int M, double *Lout)
{
	return host_batch(s, ypred, B, s ? curve_bins(s) : 0, row_ids, M, Lout, 0, fn_muse, "mdns_muse_loglike_batch");
}
extern "C" int mdns_muse3_loglike_batch(mdns_spectra *s, const double *params, int B,
                                        const int *row_ids, int M, double *Lout)
{
	return host_batch(s, params, B, 5, row_ids, M, Lout, 0, fn_muse3, "mdns_muse3_loglike_batch");
}
extern "C" int mdns_lines_loglike_batch(mdns_spectra *s, const double *params, int B,
                                        const int *row_ids, int M, double *Lout)
{
	return host_batch(s, params, B, s ? muse_nparams(s) : 0, row_ids, M, Lout, 0, fn_lines, "mdns_lines_loglike_batch");
}

// the templates themselves: out [B][nx] on the host
extern "C" int mdns_lines_template_batch(mdns_spectra *s, const double *params, int B, double *out)
{
	Context *c = ctx();
	if (!c) return 1;
	if (!s || !params || !out || B < 0) { set_error("mdns_lines_template_batch: bad arguments (B=%d)", B); return 1; }
	if (!s->d_x.get()) { set_error("mdns_lines_template_batch: spectra were created without a wavelength grid"); return 1; }
	if (B == 0 || s->nx == 0) return 0;
	const int ldm = model_ld(s->nx);
	const size_t pbytes = (size_t) B * muse_nparams(s) * sizeof(double);
	if (!s->d_params.fit((size_t) B * muse_nparams(s))) return 1;
	if (!s->d_model.fit((size_t) B * ldm)) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(s->d_params.get(), params, pbytes, hipMemcpyHostToDevice, c->stream))) return 1;
	if (!launch_muse_model(s, s->d_params.get(), B, s->d_model.get(), ldm)) return 1;
	if (!MDNS_HIP(hipMemcpy2DAsync(out, (size_t) s->nx * sizeof(double), s->d_model.get(), (size_t) ldm * sizeof(double),
	                               (size_t) s->nx * sizeof(double), (size_t) B, hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}

// ---------------------------------------------------------------------------------------
// drop-in likelihood entry points (reference argument lists)
// ---------------------------------------------------------------------------------------
struct Registered {
	const void *yy; const void *vv; int ndata; int nx; mdns_spectra *s;
};
static std::vector<Registered> g_registered;

static mdns_spectra *find_registered(const void *yy, const void *vv, int ndata, int nx)
{
	for (const Registered &r : g_registered)
		if (r.yy == yy && r.ndata == ndata && r.nx == nx && (vv == nullptr || r.vv == vv)) return r.s;
	return nullptr;
}

extern "C" int mdns_register_spectra(const void *yy, const void *vv, int ndata, int nx)
{
	mdns_unregister_spectra(yy);
	mdns_spectra *s = mdns_spectra_create(nullptr, (const double *) yy, (const double *) vv, ndata, nx,
	                                      MDNS_LAYOUT_CHANNEL_MAJOR);
	if (!s) return 1;
	g_registered.push_back(Registered{yy, vv, ndata, nx, s});
	return 0;
}

extern "C" int mdns_unregister_spectra(const void *yy)
{
	for (size_t i = 0; i < g_registered.size(); i++)
		if (g_registered[i].yy == yy) {
			mdns_spectra_destroy(g_registered[i].s);
			g_registered.erase(g_registered.begin() + i);
			return 0;
		}
	return 1;
}

// MDNS_ASSUME_STATIC_SPECTRA=1: the drop-in like() calls register every spectra array they
// see (by pointer and shape) instead of uploading it on each call -- for hosts such as the
// reference's sample.py / musefuse.py, which load their data once and never modify it
static bool assume_static_spectra()
{
	static const char *e = getenv("MDNS_ASSUME_STATIC_SPECTRA");
	return e && *e && *e != '0';
}

// mask (C bool per data set) -> ascending row ids; returns the count
static int mask_to_rows(const void *data_mask, int ndata, std::vector<int> &rows)
{
	const unsigned char *m = (const unsigned char *) data_mask;
	rows.clear();
	for (int i = 0; i < ndata; i++) if (m[i]) rows.push_back(i);
	return (int) rows.size();
}

extern "C" int mdns_gauss_like(const void *xp, const void *yyp, int ndata, int nx,
                               double A, double mu, double sig, double noise_level,
                               const void *data_maskp, void *Loutp)
{
	if (!ctx()) return 1;
	std::vector<int> rows;
	const int M = mask_to_rows(data_maskp, ndata, rows);
	if (M == 0 || nx <= 0) return 0;
	mdns_spectra *s = find_registered(yyp, nullptr, ndata, nx);
	if (!s && assume_static_spectra() && mdns_register_spectra(yyp, nullptr, ndata, nx) == 0)
		s = find_registered(yyp, nullptr, ndata, nx);
	const bool temporary = (s == nullptr);
	if (temporary) {
		s = mdns_spectra_create((const double *) xp, (const double *) yyp, nullptr, ndata, nx,
		                        MDNS_LAYOUT_CHANNEL_MAJOR);
		if (!s) return 1;
	} else {
		// the grid belongs to the call, not to the registration (clike.c:35 takes x every call)
		Context *c = ctx();
		if (!s->d_x.get() && !s->d_x.make((size_t) nx)) return 1;
		if (!MDNS_HIP(hipMemcpyAsync(s->d_x.get(), xp, nx * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
		if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
	}
	const double params[3] = {A, mu, sig};
	std::vector<double> L((size_t) M);
	int rc = mdns_gauss_loglike_batch(s, params, 1, noise_level, M == ndata ? nullptr : rows.data(), M, L.data());
	if (temporary) mdns_spectra_destroy(s);
	if (rc != 0) return rc;
	// clike.c:72 accumulates the raw sums  sum_j ((m_j - y_ij)/noise)^2 = -2 * loglike
	double *Lout = (double *) Loutp;
	for (int k = 0; k < M; k++) Lout[k] += -2.0 * L[k];
	return 0;
}

extern "C" int mdns_muse_like(const void *yyp, const void *vvp, const void *ypredp,
                              const void *data_maskp, int ndata, int nx, void *Loutp)
{
	if (!ctx()) return 1;
	std::vector<int> rows;
	const int M = mask_to_rows(data_maskp, ndata, rows);
	if (M == 0) return 0;
	mdns_spectra *s = find_registered(yyp, vvp, ndata, nx);
	if (!s && assume_static_spectra() && mdns_register_spectra(yyp, vvp, ndata, nx) == 0)
		s = find_registered(yyp, vvp, ndata, nx);
	const bool temporary = (s == nullptr);
	if (temporary) {
		s = mdns_spectra_create(nullptr, (const double *) yyp, (const double *) vvp, ndata, nx,
		                        MDNS_LAYOUT_CHANNEL_MAJOR);
		if (!s) return 1;
	}
	std::vector<double> L((size_t) M);
	int rc = mdns_muse_loglike_batch(s, (const double *) ypredp, 1, M == ndata ? nullptr : rows.data(), M, L.data());
	if (temporary) mdns_spectra_destroy(s);
	if (rc != 0) return rc;
	double *Lout = (double *) Loutp;          // not compacted; unmasked entries untouched
	for (int k = 0; k < M; k++) Lout[rows[k]] = L[k];
	return 0;
}

// ---------------------------------------------------------------------------------------
// drop-in neighbourhood entry points
// ---------------------------------------------------------------------------------------
extern "C" int mdns_count_within_dev(const double *d_members, int K, int ndim, double maxdistance,
                                     const double *d_cands, int M, int *d_counts)
{
	Context *c = ctx();
	if (!c) return 1;
	if (K < 0 || M < 0 || ndim <= 0) { set_error("mdns_count_within_dev: bad sizes"); return 1; }
	if (M == 0) return 0;
	if (K == 0) return MDNS_HIP(hipMemsetAsync(d_counts, 0, (size_t) M * sizeof(int), c->stream)) ? 0 : 1;
	return launch_count_within(d_members, K, ndim, sqrt_threshold(maxdistance), nullptr, d_cands, M, d_counts) ? 0 : 1;
}

extern "C" int mdns_bootstrap_round_maxsq_dev(const double *d_members, int K, int ndim,
                                              const double *d_chosen, int nbootstraps,
                                              double *d_round_sq)
{
	Context *c = ctx();
	if (!c) return 1;
	if (K < 0 || nbootstraps < 0 || ndim <= 0) { set_error("mdns_bootstrap_round_maxsq_dev: bad sizes"); return 1; }
	if (nbootstraps == 0) return 0;
	// k_pack_chosen clears d_round_sq itself; an empty pool still has to report zeros
	if (K == 0) return MDNS_HIP(hipMemsetAsync(d_round_sq, 0, (size_t) nbootstraps * sizeof(double), c->stream)) ? 0 : 1;
	return launch_bootstrap(d_members, K, ndim, d_chosen, nbootstraps, d_round_sq) ? 0 : 1;
}

// upload a few host arrays into the context's device scratch (16-byte aligned slots) and
// hand back the device pointers; one H2D per array on the library stream
static bool stage_in(const void *const *src, const size_t *bytes, int n, size_t extra_bytes, char **d_ptrs,
                     char **d_extra)
{
	Context *c = ctx();
	size_t total = 0;
	for (int i = 0; i < n; i++) total += (bytes[i] + 255) & ~(size_t) 255;
	char *base = (char *) device_scratch(total + extra_bytes + 256);
	if (!base) return false;
	size_t off = 0;
	for (int i = 0; i < n; i++) {
		d_ptrs[i] = base + off;
		if (bytes[i] && !MDNS_HIP(hipMemcpyAsync(d_ptrs[i], src[i], bytes[i], hipMemcpyHostToDevice, c->stream)))
			return false;
		off += (bytes[i] + 255) & ~(size_t) 255;
	}
	*d_extra = base + off;
	return true;
}

extern "C" int mdns_count_within_distance_of(const void *xx, int nsamples, int ndim, double maxdistance,
                                             const void *yy, int nothers, void *outp, const int countmax)
{
	Context *c = ctx();
	if (!c) return 1;
	if (nothers <= 0) return 0;
	if (nsamples <= 0) return 0;               // no member: nothing is incremented
	if (ndim <= 0) { set_error("mdns_count_within_distance_of: ndim=%d", ndim); return 1; }
	const void *src[2] = {xx, yy};
	const size_t bytes[2] = {(size_t) nsamples * ndim * 8, (size_t) nothers * ndim * 8};
	char *d[2], *d_counts;
	if (!stage_in(src, bytes, 2, (size_t) nothers * 4, d, &d_counts)) return 1;
	if (mdns_count_within_dev((const double *) d[0], nsamples, ndim, maxdistance, (const double *) d[1],
	                          nothers, (int *) d_counts) != 0) return 1;
	std::vector<int> hits((size_t) nothers);
	if (!MDNS_HIP(hipMemcpyAsync(hits.data(), d_counts, (size_t) nothers * 4, hipMemcpyDeviceToHost, c->stream))) return 1;
	if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return 1;
	// cneighbors.c:108-115: out[j]++ per member inside, scanning stops once out[j] >= countmax
	double *out = (double *) outp;
	for (int j = 0; j < nothers; j++) {
		int h = hits[j];
		if (countmax > 0) {
			while (h > 0) { out[j] += 1; h--; if (out[j] >= countmax) break; }
		} else {
			for (; h > 0; h--) out[j] += 1;
		}
	}
	return 0;
}

extern "C" int mdns_is_within_distance_of(const void *xx, int nsamples, int ndim, double maxdistance,
                                          const void *y)
{
	double out = 0;
	if (nsamples <= 0) return 0;
	if (mdns_count_within_distance_of(xx, nsamples, ndim, maxdistance, y, 1, &out, 1) != 0) return -1;
	return out > 0 ? 1 : 0;
}

extern "C" double mdns_bootstrapped_maxdistance(const void *xx, int nsamples, int ndim,
                                                const void *choice, int nbootstraps)
{
	Context *c = ctx();
	if (!c) return NAN;
	if (nsamples <= 0 || nbootstraps <= 0 || ndim <= 0) {
		set_error("mdns_bootstrapped_maxdistance: bad sizes (%d, %d, %d)", nsamples, ndim, nbootstraps);
		return NAN;
	}
	const void *src[2] = {xx, choice};
	const size_t bytes[2] = {(size_t) nsamples * ndim * 8, (size_t) nsamples * nbootstraps * 8};
	char *d[2], *d_round;
	if (!stage_in(src, bytes, 2, (size_t) nbootstraps * 8, d, &d_round)) return NAN;
	if (mdns_bootstrap_round_maxsq_dev((const double *) d[0], nsamples, ndim, (const double *) d[1],
	                                   nbootstraps, (double *) d_round) != 0) return NAN;
	std::vector<double> sq((size_t) nbootstraps);
	if (!MDNS_HIP(hipMemcpyAsync(sq.data(), d_round, (size_t) nbootstraps * 8, hipMemcpyDeviceToHost, c->stream))) return NAN;
	if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return NAN;
	// sqrt is monotone: max_i sqrt(min_j d_ij) = sqrt(max_i min_j d_ij) (cneighbors.c:160-174)
	double best = 0;
	for (int b = 0; b < nbootstraps; b++) { const double r = std::sqrt(sq[b]); if (r > best) best = r; }
	return best;
}

extern "C" double mdns_most_distant_nearest_neighbor(const void *xx, int nsamples, int ndim)
{
	Context *c = ctx();
	if (!c) return NAN;
	if (nsamples <= 0 || ndim <= 0) { set_error("mdns_most_distant_nearest_neighbor: bad sizes"); return NAN; }
	const void *src[1] = {xx};
	const size_t bytes[1] = {(size_t) nsamples * ndim * 8};
	char *d[1], *d_out;
	if (!stage_in(src, bytes, 1, 8, d, &d_out)) return NAN;
	if (!MDNS_HIP(hipMemsetAsync(d_out, 0, 8, c->stream))) return NAN;
	if (!launch_nn_maxsq((const double *) d[0], nsamples, ndim, (double *) d_out)) return NAN;
	double sq = 0;
	if (!MDNS_HIP(hipMemcpyAsync(&sq, d_out, 8, hipMemcpyDeviceToHost, c->stream))) return NAN;
	if (!MDNS_HIP(hipStreamSynchronize(c->stream))) return NAN;
	return std::sqrt(sq);
}

// ---------------------------------------------------------------------------------------
// resident RadFriends region (members + radius)
// ---------------------------------------------------------------------------------------
// Device buffers of the region handles come from a small cache: the host code builds a region
// per rebuild of a constrained draw (thousands per run), and hipMalloc / hipFree per buffer were a
// quarter of a millisecond per region.  Everything runs on one stream, so a buffer handed back
// and taken again is reused in stream order: no synchronisation is needed.
struct PoolEntry { size_t bytes; void *p; };
static std::vector<PoolEntry> g_pool;

static void *pool_take(size_t bytes, size_t *got)
{
	size_t want = 4096;
	while (want < bytes) want <<= 1;
	for (size_t i = 0; i < g_pool.size(); i++)
		if (g_pool[i].bytes == want) {
			void *p = g_pool[i].p;
			g_pool[i] = g_pool.back();
			g_pool.pop_back();
			*got = want;
			return p;
		}
	void *p = nullptr;
	if (!MDNS_HIP(hipMalloc(&p, want))) return nullptr;
	*got = want;
	return p;
}

static void pool_give(void *p, size_t bytes)
{
	if (!p) return;
	if (g_pool.size() >= 64) { (void) hipFree(p); return; }
	g_pool.push_back({bytes, p});
}

// A block taken from the pool; it goes back there with its owner.
struct PoolBlock {
	void *p = nullptr;
	size_t bytes = 0;
	PoolBlock() = default;
	PoolBlock(const PoolBlock &) = delete;
	PoolBlock &operator=(const PoolBlock &) = delete;
	~PoolBlock() { pool_give(p, bytes); }
	// holds at least `need` bytes afterwards (contents are not kept); false (error set): the block is empty
	bool fit(size_t need)
	{
		if (need <= bytes) return true;
		pool_give(p, bytes);
		bytes = 0;
		p = pool_take(need, &bytes);
		return p != nullptr;
	}
};

struct mdns_region {
	const double *d_members = nullptr;
	PoolBlock owned;                  // the members, when this handle allocated them
	int K = 0, ndim = 0;
	double radius = NAN;              // maxdistance, host copy
	double thresh_sq = NAN;           // membership threshold on squared distances, host copy
	// A radius computation ends on the device: the last workgroup of the bootstrap kernel
	// writes {radius, threshold} to d_res (for the membership kernel, stream order) and to
	// h_res (mapped host memory), then h_res->seq = seq.  The host polls for that.
	double *d_round = nullptr;        // per-round max of squared nearest-chosen distances (slab or own_round)
	PoolBlock own_round;
	int round_cap = 0;
	RegionResult *d_res = nullptr;
	RegionResult *h_res = nullptr;    // hipHostMalloc (mapped, coherent)
	RegionResult *h_res_dev = nullptr;   // its device address
	unsigned *d_counter = nullptr;
	int slot = -1;                    // result slot (take_result_slot)
	unsigned long long seq = 0;
	bool on_device = false;           // the membership kernel must use d_res
	bool pending = false;             // the host copies still have to be fetched (async path)
	PoolBlock d_chosen, d_points, d_counts;
};

// Result slots ({radius, threshold} on the device, its mapped host mirror and the ticket
// counter) come from slabs allocated once: the host code builds a region handle per region,
// and hipHostMalloc per handle was a millisecond each.
static constexpr int kSlabSlots = 64;
static constexpr int kSlotRounds = 16;    // per-round maxima kept in the slab (more: own buffer)
struct ResultSlab {
	DeviceBuffer<RegionResult> d_res;
	DeviceBuffer<unsigned> d_counter;
	DeviceBuffer<double> d_round;
	PinnedBuffer h_res{hipHostMallocMapped | hipHostMallocCoherent};
};
// kept for the life of the process and, like the context, never destroyed: owners must not free through a runtime
// that is being torn down at exit
static std::vector<ResultSlab> &g_slabs = *new std::vector<ResultSlab>;
static std::vector<int> g_free_slots;

static int take_result_slot()
{
	if (g_free_slots.empty()) {
		// (a slab that fails part-way frees what it made on return: nothing is left behind, g_slabs does not grow)
		ResultSlab slab;
		if (!slab.d_res.make(kSlabSlots) || !slab.d_counter.make(kSlabSlots, true) ||
		    !slab.d_round.make(kSlabSlots * kSlotRounds, true) || !slab.h_res.make(kSlabSlots * sizeof(RegionResult))) return -1;
		const int base = (int) g_slabs.size() * kSlabSlots;
		g_slabs.push_back(std::move(slab));
		for (int i = kSlabSlots - 1; i >= 0; i--) g_free_slots.push_back(base + i);
	}
	const int slot = g_free_slots.back();
	g_free_slots.pop_back();
	return slot;
}

static bool region_fetch(mdns_region *r);

// *started_ns: 0 before the first call of a wait
static bool poll_expired(long long *started_ns)
{
	static const double limit_s = [] { const char *v = getenv("MDNS_POLL_TIMEOUT_S"); const double t = v ? atof(v) : 120.0; return t > 0 ? t : 120.0; }();
	struct timespec ts;
	clock_gettime(CLOCK_MONOTONIC, &ts);
	const long long now = (long long) ts.tv_sec * 1000000000LL + ts.tv_nsec;
	if (*started_ns == 0) { *started_ns = now; return false; }
	return (double) (now - *started_ns) * 1e-9 > limit_s;
}

Wait mdns::wait_seq(const volatile unsigned long long *at, unsigned long long want, hipError_t *err)
{
	// The number usually is there already (the caller has launched other work meanwhile).
	// While polling, look at the stream now and then: once it has drained, everything the
	// kernel wrote is visible, and a failed launch shows up as an error instead of a hang.
	long long started = 0;
	for (unsigned spin = 0; *at != want; spin++) {
		if ((spin & 1023) != 1023) continue;
		const hipError_t e = hipStreamQuery(g_ctx.stream);
		if (e == hipErrorNotReady) {
			if (poll_expired(&started)) return Wait::timeout;
			continue;
		}
		if (e != hipSuccess) {
			if (err) *err = e;
			return Wait::failed;
		}
		if (*at != want) return Wait::empty;
	}
	std::atomic_thread_fence(std::memory_order_acquire);
	return Wait::ok;
}

bool mdns::wait_ok(Wait w, hipError_t err, const char *who)
{
	switch (w) {
	case Wait::ok: return true;
	case Wait::timeout: set_error("%s: no result within MDNS_POLL_TIMEOUT_S", who); break;
	case Wait::failed: set_error("%s failed: %s", who, hipGetErrorString(err)); break;
	case Wait::empty: set_error("%s finished without a result", who); break;
	}
	return false;
}

// A radius computation on r's members into r's result slot: `launch` is launch_bootstrap (choice matrix) or
// launch_bootstrap_packed (bit masks).  Once it is in the stream the membership kernel takes its threshold from
// d_res, and the host copies are to be fetched under the new `seq`.
template <class Choice>
static bool region_launch_radius(mdns_region *r, bool (*launch)(const double *, int, int, const Choice *, int, double *, const BootstrapFinish *),
                                 const Choice *d_choice, int nbootstraps)
{
	const BootstrapFinish fin = {r->d_counter, r->d_res, r->h_res_dev, ++r->seq};
	if (!launch(r->d_members, r->K, r->ndim, d_choice, nbootstraps, r->d_round, &fin)) return false;
	r->on_device = true;
	r->pending = true;
	return true;
}

// d_members == nullptr: the members are the region's own block (r->owned, filled by the caller)
static bool region_init(mdns_region *r, const double *d_members, int K, int ndim)
{
	r->d_members = d_members ? d_members : (const double *) r->owned.p; r->K = K; r->ndim = ndim;
	r->slot = take_result_slot();
	if (r->slot < 0) return false;
	const ResultSlab &slab = g_slabs[r->slot / kSlabSlots];
	const int i = r->slot % kSlabSlots;
	r->d_res = slab.d_res.get() + i;
	r->d_counter = slab.d_counter.get() + i;
	r->h_res = (RegionResult *) slab.h_res.get() + i;
	r->h_res_dev = (RegionResult *) slab.h_res.dev() + i;
	r->d_round = slab.d_round.get() + (size_t) i * kSlotRounds;      // zero: every finishing computation leaves it so
	r->round_cap = kSlotRounds;
	r->seq = r->h_res->seq;            // a recycled slot keeps counting from where it was
	return true;
}

extern "C" mdns_region *mdns_region_create(const double *members, int K, int ndim)
{
	Context *c = ctx();
	if (!c) return nullptr;
	if (!members || K <= 0 || ndim <= 0) { set_error("mdns_region_create: bad arguments (K=%d ndim=%d)", K, ndim); return nullptr; }
	const size_t bytes = (size_t) K * ndim * sizeof(double);
	mdns_region *r = new mdns_region();
	if (!r->owned.fit(bytes) ||
	    !MDNS_HIP(hipMemcpyAsync(r->owned.p, members, bytes, hipMemcpyHostToDevice, c->stream)) ||
	    !MDNS_HIP(hipStreamSynchronize(c->stream)) ||
	    !region_init(r, nullptr, K, ndim)) { mdns_region_destroy(r); return nullptr; }
	return r;
}

// Members and packed bootstrap choice staged together, K6 launched, radius waited for: what
// RadFriendsRegion.__init__ (radfriendsregion.py:59-70) needs from the device, in ONE call --
// one pinned staging copy, one H2D, one launch, one poll of the mapped result.
// wait == false: the radius stays in flight (mdns_region_radius waits for it); the pinned staging
// block is busy until then -- the caller creates no other region meanwhile
static mdns_region *create_bootstrapped(const double *members, int K, int ndim, const unsigned *packed, int nbootstraps,
                                        double *radius, bool wait)
{
	Context *c = ctx();
	if (!c) return nullptr;
	if (!members || !packed || (wait && !radius) || K <= 0 || ndim <= 0 || nbootstraps <= 0 || nbootstraps > 16) {
		set_error("mdns_region_create_bootstrapped: bad arguments (K=%d ndim=%d rounds=%d)", K, ndim, nbootstraps);
		return nullptr;
	}
	const size_t mbytes = (size_t) K * ndim * sizeof(double), pbytes = (size_t) K * sizeof(unsigned);
	const size_t poff = (mbytes + 255) & ~(size_t) 255;
	mdns_region *r = new mdns_region();
	char *pin = r->owned.fit(poff + pbytes) ? (char *) pinned_scratch(poff + pbytes) : nullptr;
	if (!pin) { mdns_region_destroy(r); return nullptr; }
	char *const d = (char *) r->owned.p;
	memcpy(pin, members, mbytes);
	memcpy(pin + poff, packed, pbytes);
	if (!MDNS_HIP(hipMemcpyAsync(d, pin, poff + pbytes, hipMemcpyHostToDevice, c->stream))) { mdns_region_destroy(r); return nullptr; }
	if (!region_init(r, nullptr, K, ndim) ||
	    !region_launch_radius(r, launch_bootstrap_packed, (const unsigned *) (d + poff), nbootstraps)) {
		(void) hipStreamSynchronize(c->stream);
		mdns_region_destroy(r);
		return nullptr;
	}
	if (!wait) return r;
	*radius = mdns_region_radius(r);          // waits: the pinned staging block is free again
	if (*radius != *radius) { mdns_region_destroy(r); return nullptr; }
	return r;
}

extern "C" mdns_region *mdns_region_create_bootstrapped(const double *members, int K, int ndim,
                                                        const unsigned *packed, int nbootstraps, double *radius)
{
	return create_bootstrapped(members, K, ndim, packed, nbootstraps, radius, true);
}

mdns_region *mdns::region_begin_bootstrapped(const double *members, int K, int ndim, const unsigned *packed, int nbootstraps)
{
	return create_bootstrapped(members, K, ndim, packed, nbootstraps, nullptr, false);
}

// what the chain kernels (mdns_chain.hip) need of a region whose radius is being computed or known on
// the device
bool mdns::region_view(mdns_region *r, RegionView *out)
{
	if (!r || !out || !r->on_device) return false;
	out->d_members = r->d_members; out->K = r->K; out->ndim = r->ndim; out->d_res = r->d_res;
	return true;
}

extern "C" mdns_region *mdns_region_wrap_dev(const double *d_members, int K, int ndim)
{
	if (!ctx()) return nullptr;
	if (!d_members || K <= 0 || ndim <= 0) { set_error("mdns_region_wrap_dev: bad arguments"); return nullptr; }
	mdns_region *r = new mdns_region();
	if (!region_init(r, d_members, K, ndim)) { mdns_region_destroy(r); return nullptr; }
	return r;
}

extern "C" void mdns_region_destroy(mdns_region *r)
{
	if (!r) return;
	// a radius computation still in flight writes the result slot: let it land before the slot
	// can go to another handle (the buffers themselves are reused in stream order)
	if (r->pending && ctx()) (void) region_fetch(r);
	if (r->slot >= 0) g_free_slots.push_back(r->slot);
	delete r;           // (its blocks go back to the pool)
}

extern "C" int mdns_region_set_radius(mdns_region *r, double maxdistance)
{
	if (!r) { set_error("null region"); return 1; }
	// a radius computation still in flight writes this handle's result slot: let it land first
	if (r->pending && ctx()) (void) region_fetch(r);
	r->radius = maxdistance;
	r->thresh_sq = sqrt_threshold(maxdistance);
	r->on_device = false;
	r->pending = false;
	return 0;
}

// host copies of {radius, threshold}; waits for the device when they are still in flight
static bool region_fetch(mdns_region *r)
{
	if (!r->pending) return true;
	hipError_t e = hipSuccess;
	if (!wait_ok(wait_seq(&r->h_res->seq, r->seq, &e), e, "radius computation")) return false;
	r->radius = r->h_res->radius;
	r->thresh_sq = sqrt_threshold(r->radius);     // the device derived the same number (tested)
	r->pending = false;
	return true;
}

extern "C" double mdns_region_radius(mdns_region *r)
{
	if (!r || !ctx() || !region_fetch(r)) return NAN;
	return r->radius;
}

extern "C" int mdns_region_bootstrap_radius_async(mdns_region *r, const double *d_chosen, int nbootstraps)
{
	Context *c = ctx();
	if (!c || !r) return 1;
	if (nbootstraps <= 0) { set_error("mdns_region_bootstrap_radius: nbootstraps=%d", nbootstraps); return 1; }
	if (!region_fetch(r)) return 1;             // a previous result may still be travelling
	if (r->round_cap < nbootstraps) {
		if (!r->own_round.fit((size_t) nbootstraps * sizeof(double))) return 1;
		r->d_round = (double *) r->own_round.p;
		// zero once: every finishing computation hands its slots back zeroed
		if (!MDNS_HIP(hipMemsetAsync(r->d_round, 0, (size_t) nbootstraps * sizeof(double), c->stream))) return 1;
		r->round_cap = nbootstraps;
	}
	return region_launch_radius(r, launch_bootstrap, d_chosen, nbootstraps) ? 0 : 1;
}

extern "C" double mdns_region_bootstrap_radius_dev(mdns_region *r, const double *d_chosen, int nbootstraps)
{
	if (mdns_region_bootstrap_radius_async(r, d_chosen, nbootstraps) != 0) return NAN;
	return mdns_region_radius(r);
}

extern "C" double mdns_region_bootstrap_radius(mdns_region *r, const double *chosen, int nbootstraps)
{
	Context *c = ctx();
	if (!c || !r) return NAN;
	const size_t n = (size_t) r->K * (nbootstraps > 0 ? nbootstraps : 0);
	if (n == 0) { set_error("mdns_region_bootstrap_radius: nbootstraps=%d", nbootstraps); return NAN; }
	if (!r->d_chosen.fit(n * sizeof(double))) return NAN;
	if (!MDNS_HIP(hipMemcpyAsync(r->d_chosen.p, chosen, n * sizeof(double), hipMemcpyHostToDevice, c->stream))) return NAN;
	return mdns_region_bootstrap_radius_dev(r, (const double *) r->d_chosen.p, nbootstraps);
}

extern "C" double mdns_region_bootstrap_radius_packed(mdns_region *r, const unsigned *packed, int nbootstraps)
{
	Context *c = ctx();
	if (!c || !r) return NAN;
	if (nbootstraps <= 0 || nbootstraps > 16 || !packed) { set_error("mdns_region_bootstrap_radius_packed: nbootstraps=%d (1..16)", nbootstraps); return NAN; }
	if (!region_fetch(r)) return NAN;
	const size_t bytes = (size_t) r->K * sizeof(unsigned);
	if (!r->d_chosen.fit(bytes)) return NAN;
	if (!MDNS_HIP(hipMemcpyAsync(r->d_chosen.p, packed, bytes, hipMemcpyHostToDevice, c->stream))) return NAN;
	if (!region_launch_radius(r, launch_bootstrap_packed, (const unsigned *) r->d_chosen.p, nbootstraps)) return NAN;
	return mdns_region_radius(r);
}

extern "C" int mdns_region_count_dev(mdns_region *r, const double *d_points, int M, int *d_counts)
{
	if (!ctx() || !r) return 1;
	if (M < 0) { set_error("mdns_region_count: M=%d", M); return 1; }
	if (M == 0) return 0;
	if (!r->on_device && r->radius != r->radius) { set_error("mdns_region_count: the region has no radius yet"); return 1; }
	// right after a radius computation the kernel takes the threshold the bootstrap kernel
	// left in device memory (stream order)
	return launch_count_within(r->d_members, r->K, r->ndim, r->thresh_sq, r->on_device ? r->d_res : nullptr,
	                           d_points, M, d_counts) ? 0 : 1;
}

// one staging block for the membership round trips of the native constrainer: pinned + mapped,
// layout { seq | counts int32[M] | points f64[M * ndim] } (Context::count_stage; count_ticket: workgroups of the
// current launch that are through)
static unsigned long long g_stage_seq = 0;

// K3 for host points with the least round trip: ONE kernel.  The points sit in a pinned block mapped
// into the device, the kernel reads them there, stores the counts there and its last workgroup
// raises a sequence number the host polls for.  (History, per call in a real run: pageable copies
// both ways and a stream synchronisation 42 us; pinned copy in + count + export kernel + polling
// 35 us, of which four device commands -- copy, clear, count, export -- for 6 us of counting.
// Tried: member chunks adding partial counts in a device buffer that the last workgroup exports and
// clears -- more workgroups, but 2.17 s against 1.65-1.73 s over the 73 600 calls of a C2 run.)
extern "C" int mdns_region_count_polled(mdns_region *r, const double *points, int M, int *counts)
{
	Context *c = ctx();
	if (!c || !r) return 1;
	if (M <= 0) return M < 0;
	if (!r->on_device && r->radius != r->radius) { set_error("mdns_region_count: the region has no radius yet"); return 1; }
	const size_t n = (size_t) M * r->ndim;
	// (the layout follows M, not the capacity: nothing in the block outlives a call but its first word)
	const size_t off_counts = 64, off_points = (64 + (size_t) M * sizeof(int) + 63) & ~(size_t) 63;
	if (!c->count_ticket.fit_zeroed(1)) return 1;
	const size_t had = c->count_stage.cap();
	if (!c->count_stage.fit(off_points + n * sizeof(double))) return 1;
	char *const stage = c->count_stage.get(), *const stage_dev = c->count_stage.dev();
	int *const ticket = c->count_ticket.get();
	if (c->count_stage.cap() != had) *(volatile unsigned long long *) stage = g_stage_seq;      // a new block: its number so far
	memcpy(stage + off_points, points, n * sizeof(double));
	const unsigned long long seq = ++g_stage_seq;
	const CountMail mail = {ticket, (unsigned long long *) stage_dev, seq};
	// right after a radius computation the kernel takes the threshold the bootstrap kernel left in
	// device memory (stream order)
	if (!launch_count_within(r->d_members, r->K, r->ndim, r->thresh_sq, r->on_device ? r->d_res : nullptr,
	                         (const double *) (stage_dev + off_points), M, (int *) (stage_dev + off_counts), &mail)) return 1;
	hipError_t e = hipSuccess;
	const Wait w = wait_seq((const volatile unsigned long long *) stage, seq, &e);
	// (the stream drained and the number is not there: the launch failed; the ticket counter may be anywhere)
	if (w == Wait::empty) (void) hipMemsetAsync(ticket, 0, sizeof(int), c->stream);
	if (!wait_ok(w, e, "membership count")) return 1;
	memcpy(counts, stage + off_counts, (size_t) M * sizeof(int));
	return 0;
}

extern "C" int mdns_region_count(mdns_region *r, const double *points, int M, int *counts)
{
	Context *c = ctx();
	if (!c || !r) return 1;
	if (M <= 0) return M < 0;
	const size_t n = (size_t) M * r->ndim;
	if (!r->d_points.fit(n * sizeof(double)) || !r->d_counts.fit((size_t) M * sizeof(int))) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(r->d_points.p, points, n * sizeof(double), hipMemcpyHostToDevice, c->stream))) return 1;
	if (mdns_region_count_dev(r, (const double *) r->d_points.p, M, (int *) r->d_counts.p) != 0) return 1;
	if (!MDNS_HIP(hipMemcpyAsync(counts, r->d_counts.p, (size_t) M * sizeof(int), hipMemcpyDeviceToHost, c->stream))) return 1;
	return MDNS_HIP(hipStreamSynchronize(c->stream)) ? 0 : 1;
}
