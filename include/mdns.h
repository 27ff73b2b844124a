/*
 * mdns.h -- C ABI of libmdns_hip.so, the MI355X (gfx950) implementation of the
 * massivedatans hot path: batched spectral-line log-likelihoods and the RadFriends
 * neighbourhood / safe-radius tests.
 *
 * Plain C: pointers and sizes only, no C++ or torch types.  Every entry point names the
 * reference interface it stands in for (paths under the reference checkout).
 *
 * The library has NO CPU fallback: every compute entry point runs HIP kernels on the
 * selected device and reports failure (return code / NaN, message via mdns_last_error())
 * when no device is usable.
 *
 * Threading: like the reference (one Python thread; its OpenMP lives inside the .so files),
 * the entry points are meant to be called from one thread at a time.  One process drives one
 * GPU; all work is issued on one HIP stream (the library's own, or the caller's through
 * mdns_set_stream).
 *
 * Part 1  drop-in entry points with the reference's argument lists (host pointers);
 *         the three shim libraries clike.so / cmuselike.so / cneighbors.so re-export them
 *         under the reference's symbol names.
 * Part 2  device-resident handles (spectra stay in HBM, candidates are scored in batches).
 * Part 3  raw device entry points, memory, stream and event helpers (bench / multi-GPU).
 */
#ifndef MDNS_H
#define MDNS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------ */
/* Library state                                                                        */
/* ------------------------------------------------------------------------------------ */

/* Select the device of this process (one process per GPU).  device < 0: MDNS_DEVICE, else
 * LOCAL_RANK modulo the device count, else 0.  Called implicitly by the first compute call.
 * Returns 0 on success. */
int mdns_init(int device);
/* Number of visible HIP devices (0 when there is none). */
int mdns_device_count(void);
/* Message of the last failure in this thread's process ("" if none). */
const char *mdns_last_error(void);
/* ABI version, bumped on any signature change. */
int mdns_abi_version(void);

/* ------------------------------------------------------------------------------------ */
/* Part 1: drop-in entry points (reference argument lists, host pointers)               */
/* ------------------------------------------------------------------------------------ */

/*
 * K1 -- stands in for `like` of clike.so: clike.c:34-40, bound at sample.py:85-96, called at
 * sample.py:106.  x f64[nx]; yy f64[nx,ndata] C-order (element (j,i) at i + j*ndata);
 * data_mask C bool[ndata]; Lout f64[mask.sum()], compacted in mask order and ACCUMULATED
 * (+=, clike.c:72) -- the caller pre-zeroes it (sample.py:104).  Returns 0 (the reference
 * always does); non-zero only on a device failure.
 * The spectra are uploaded on every call unless the yy pointer was registered with
 * mdns_register_spectra() (then the HBM-resident copy is used).
 */
int mdns_gauss_like(const void *x, const void *yy, int ndata, int nx,
                    double A, double mu, double sig, double noise_level,
                    const void *data_mask, void *Lout);

/*
 * K2 -- stands in for `like` of cmuselike.so: cmuselike.c:34-38, bound at
 * musefuse.py:509-517, called at musefuse.py:534.  yy, vv f64[nx,ndata]; ypred f64[nx];
 * Lout f64[ndata] NOT compacted, only masked entries are written (cmuselike.c:49,62).
 */
int mdns_muse_like(const void *yy, const void *vv, const void *ypred, const void *data_mask,
                   int ndata, int nx, void *Lout);

/* Keep a device copy of a host spectra array for the drop-in calls above: later calls whose
 * yy (and vv) pointer, ndata and nx match use it instead of uploading.  The caller promises
 * not to modify the array while it is registered.  vv may be NULL (K1). */
int mdns_register_spectra(const void *yy, const void *vv, int ndata, int nx);
int mdns_unregister_spectra(const void *yy);

/* K5 -- cneighbors.c:32-34 (clustering/neighbors.py:100-110). */
double mdns_most_distant_nearest_neighbor(const void *xx, int nsamples, int ndim);
/* K4 -- cneighbors.c:77-79 (clustering/neighbors.py:112-124); 1 = inside. */
int mdns_is_within_distance_of(const void *xx, int nsamples, int ndim, double maxdistance,
                               const void *y);
/* K3 -- cneighbors.c:95-98 (clustering/neighbors.py:126-159).  out f64[nothers] is
 * incremented in place, with the reference's countmax early-stop semantics. */
int mdns_count_within_distance_of(const void *xx, int nsamples, int ndim, double maxdistance,
                                  const void *yy, int nothers, void *out, const int countmax);
/* K6 -- cneighbors.c:125-130 (clustering/neighbors.py:161-177).  choice f64[nsamples,
 * nbootstraps], tested != 0. */
double mdns_bootstrapped_maxdistance(const void *xx, int nsamples, int ndim,
                                     const void *choice, int nbootstraps);

/* ------------------------------------------------------------------------------------ */
/* Part 2: device-resident spectra + batched scoring (extension)        */
/* ------------------------------------------------------------------------------------ */

typedef struct mdns_spectra mdns_spectra;

#define MDNS_LAYOUT_CHANNEL_MAJOR 0   /* reference layout [nx, ndata] (sample.py:31)        */
#define MDNS_LAYOUT_DATASET_MAJOR 1   /* [ndata, nx]: one spectrum per contiguous row        */

/* Upload spectra once; they stay in HBM as [ndata, nx] rows.  x f64[nx] (may be NULL when
 * only precomputed templates are scored); v per-pixel variances (NULL for K1-only use). */
mdns_spectra *mdns_spectra_create(const double *x, const double *y, const double *v,
                                  int ndata, int nx, int layout);
void mdns_spectra_destroy(mdns_spectra *s);
int mdns_spectra_ndata(const mdns_spectra *s);
int mdns_spectra_nx(const mdns_spectra *s);

/*
 * Score B candidate lines against M selected spectra in one pass over the spectra.
 * params f64[B,3] = (A, mu, sig) per candidate (sig already linear, sample.py:103);
 * row_ids int32[M] = indices of the selected spectra in ascending mask order (NULL = all,
 * M = ndata); Lout f64[B,M] receives the log-likelihoods  -0.5 * sum_j ((m_j - y_ij)/noise)^2
 * (what sample.py:108 returns), compacted like the reference's output.
 */
int mdns_gauss_loglike_batch(mdns_spectra *s, const double *params, int B, double noise_level,
                             const int *row_ids, int M, double *Lout);

/* Same for the scale-marginalised likelihood (cmuselike.c:45-64) against B precomputed
 * templates ypred f64[B,nx]; Lout f64[B,M] = -0.5*chi. */
int mdns_muse_loglike_batch(mdns_spectra *s, const double *ypred, int B,
                            const int *row_ids, int M, double *Lout);

/* Config-C5 template (three Gaussians on a flat continuum, massivedatans_amd/gen.py
 * muse_template) evaluated ON DEVICE for B parameter vectors params f64[B,5], then scored
 * exactly as mdns_muse_loglike_batch. */
int mdns_muse3_loglike_batch(mdns_spectra *s, const double *params, int B,
                             const int *row_ids, int M, double *Lout);

/* The same model family with a caller-chosen line list: G rows lines f64[G,3] = (mu, a, sigma) and the index
 * ref of the line whose ratio is fixed to 1; 1 <= G <= 6, 0 <= ref < G, finite values, sigma > 0.  A candidate
 * then has G + 2 parameters (log_amp, z, log_width_scale, r_g for g != ref in ascending g) and its template is
 *   1 + 10**log_amp * sum_g r_g a_g exp(-0.5 ((x - mu_g (1+z)) / (sigma_g 10**log_width_scale))**2),  r_ref = 1
 * (massivedatans_amd/gen.py muse_template).  G = 0 clears the list: the built-in three lines, 5 parameters.
 * Everything that scores parameters on this handle -- the entry points below, mdns_joint_init_muse3, the
 * mdns_backend_draw_* chunks of a joint state over it -- takes rows of mdns_spectra_nparams(s) doubles.  The list
 * cannot change while a joint state exists on the handle (returns 1, mdns_last_error says so). */
int mdns_spectra_set_lines(mdns_spectra *s, const double *lines, int G, int ref);
/* 5 with no list set, else G + 2. */
int mdns_spectra_nparams(const mdns_spectra *s);
/* mdns_muse3_loglike_batch for the handle's model: params f64[B, mdns_spectra_nparams(s)]. */
int mdns_lines_loglike_batch(mdns_spectra *s, const double *params, int B,
                             const int *row_ids, int M, double *Lout);
/* The templates themselves, evaluated on the device: out f64[B, nx] on the host. */
int mdns_lines_template_batch(mdns_spectra *s, const double *params, int B, double *out);

/* Caller-defined models: the fixed-noise likelihood of sample.py:64-71 against B model curves the CALLER made,
 * curves f64[B][nx] (one per candidate, any model): Lout f64[B][M], Lout[b][k] = -0.5 * sum_j ((curves[b][j] -
 * y[row_k][j]) / noise_level)**2, row_ids as above.  Any spectra handle (variances are not used); nx >= 1, B >= 0,
 * M >= 0.  The value of a pair (curve, spectrum) is the same bits whatever B, M, the position of either in its
 * batch and the entry point that scored it -- one summation order over the channels (csrc/mdns_curves.hip).  Curve
 * values are not validated: non-finite ones propagate as IEEE. */
int mdns_curve_loglike_batch(mdns_spectra *s, const double *curves, int B, double noise_level,
                             const int *row_ids, int M, double *Lout);

/* Live-point pool resident on the device: the members of a RadFriends region
 * (clustering/radfriendsregion.py:59-70 keeps `members` and `maxdistance`; every are_inside /
 * count_nearby_members call of a region's life re-uses them, radfriendsregion.py:82-98).
 * Input contract of everything below (and of the cneighbors drop-ins of Part 1): member and point
 * coordinates are not NaN.  Infinite and denormal squared distances are handled as IEEE handles
 * them; a NaN distance is not -- the kernels that take minima with v_min_f64 / v_max_f64 (which
 * return the non-NaN operand) and the ones that compare would answer differently. */
typedef struct mdns_region mdns_region;

/* members f64[K, ndim] on the host (copied to the device) ... */
mdns_region *mdns_region_create(const double *members, int K, int ndim);
/* ... together with the packed bootstrap choice of its safe radius (bit b of packed[i]: point i
 * is chosen in round b, as mdns_region_bootstrap_radius_packed): one upload, one launch; *radius
 * receives the result (radfriendsregion.py:59-64 in one call). */
mdns_region *mdns_region_create_bootstrapped(const double *members, int K, int ndim,
                                             const unsigned *packed, int nbootstraps, double *radius);
/* ... or already on the device (borrowed, not copied: e.g. an all-gathered pool). */
mdns_region *mdns_region_wrap_dev(const double *d_members, int K, int ndim);
void mdns_region_destroy(mdns_region *r);
/* K6 on the resident members (cneighbors.c:125-179): chosen f64[K, nbootstraps] on the host /
 * on the device.  Returns the radius and keeps it as the region's maxdistance; NaN on failure. */
double mdns_region_bootstrap_radius(mdns_region *r, const double *chosen, int nbootstraps);
double mdns_region_bootstrap_radius_dev(mdns_region *r, const double *d_chosen, int nbootstraps);
/* The same with the choice matrix packed by the caller: bit b of packed[i] (uint32[K], host) is
 * set when point i is chosen in round b, i.e. chosen[i][b] != 0 (cneighbors.c:146); at most 16
 * rounds.  A twentieth of the bytes to build and to upload.  Bits nbootstraps..15 are ignored;
 * bits 16..31 MUST be zero (the opt-in sorted path keeps a flag of its own in bit 31).  The same
 * holds for every other `packed` argument of this header. */
double mdns_region_bootstrap_radius_packed(mdns_region *r, const unsigned *packed, int nbootstraps);
/* The same without waiting: radius and membership threshold are finished ON the device, so a
 * following mdns_region_count_dev needs no host round trip; mdns_region_radius() then waits
 * for and returns the value (the host needs it for the bounding box, radfriendsregion.py:69).
 * Returns 0 when enqueued. */
int mdns_region_bootstrap_radius_async(mdns_region *r, const double *d_chosen, int nbootstraps);
/* RadFriendsRegion(members, maxdistance=...) with a given radius (hiermetriclearn.py:54,90). */
int mdns_region_set_radius(mdns_region *r, double maxdistance);
double mdns_region_radius(mdns_region *r);
/* K3 with the region's radius (cneighbors.c:95-119, no early stop): points f64[M, ndim],
 * counts int32[M] overwritten.  Host pointers (synchronous) / device pointers (asynchronous). */
int mdns_region_count(mdns_region *r, const double *points, int M, int *counts);
int mdns_region_count_dev(mdns_region *r, const double *d_points, int M, int *d_counts);
/* mdns_region_count with the shortest round trip (what a native constrainer calls once per 1000
 * proposals): ONE kernel, which reads the points from and stores the counts to a pinned block
 * mapped into the device and raises a sequence number the host polls for -- no copies, no stream
 * synchronisation. */
int mdns_region_count_polled(mdns_region *r, const double *points, int M, int *counts);

/* ------------------------------------------------------------------------------------ */
/* Part 2b: the constrained draw decided on the device (extension) */
/* ------------------------------------------------------------------------------------ */

/*
 * The floating-point state of the joint sampler, resident in HBM: what the reference keeps in
 * `live_pointsL[nlive, ndata]` (multi_nested_sampler.py:111) and in the likelihoods of its
 * shelves (`self.shelves`, :117), plus what it derives from them on every draw -- the
 * thresholds `Lmins_higher` (:438-447: for a data set with n accepted points waiting, the
 * (n+1)-th smallest of its live and shelf likelihoods).  Everything is indexed by the ORIGINAL
 * data-set index of the spectra handle, also after data sets have finished (`cut_down`, :148-173).
 * The integer side (point ids, shelves' ids, data-set graph) stays with the host.
 */
typedef struct mdns_joint mdns_joint;

/* shelf_cap: accepted points a data set can hold waiting (grown on demand, see mdns_joint_reserve). */
mdns_joint *mdns_joint_create(mdns_spectra *s, int nlive, int shelf_cap);
void mdns_joint_destroy(mdns_joint *j);

/* Initial live points (multi_nested_sampler.py:88-103): scores params f64[nlive,3] = (A, mu, sig)
 * against ALL spectra and keeps the result as the live likelihood matrix; nothing is returned
 * (mdns_joint_get_live reads it back).  All data sets are running, all shelves empty. */
int mdns_joint_init_gauss(mdns_joint *j, const double *params, double noise_level);
/* The same for spectra with variances: params f64[nlive, mdns_spectra_nparams(s)] -- 5 of the three-line template
 * (mdns_muse3_loglike_batch), or G + 2 of the handle's line list (mdns_spectra_set_lines) -- scored with the scale-marginalised likelihood (cmuselike.c:45-64);
 * jitter f64[nlive, ndata] or NULL is added (musefuse.py:535: the tie-breaking noise the reference
 * adds to every likelihood evaluation).  A joint state over such spectra is driven through the
 * mdns_backend_* entry points (Part 5). */
int mdns_joint_init_muse3(mdns_joint *j, const double *params, const double *jitter);
/* The same from model curves the caller made, curves f64[nlive][nx], for both kinds of spectra: without variances the
 * fixed-noise likelihood (mdns_curve_loglike_batch) at noise_level, which the curve chunks of this state then use too;
 * with variances the scale-marginalised one (mdns_muse_loglike_batch; noise_level is ignored), or -- on a fixed-scale
 * handle, Part 9 -- mdns_curve_chi2_batch.  On a counts handle (Part 10; no variances, noise_level is ignored)
 * mdns_curve_poisson_batch, or -- where that handle has a background, Part 11 -- mdns_curve_wstat_batch.  jitter as
 * above. */
int mdns_joint_init_curves(mdns_joint *j, const double *curves, double noise_level, const double *jitter);
/* The same from a host matrix liveL f64[nlive, ndata] (row p = live slot p). */
int mdns_joint_set_live(mdns_joint *j, const double *liveL);
/* liveL f64[nlive, ndata] <- the device matrix (the integrator's remainder, :536-563). */
int mdns_joint_get_live(mdns_joint *j, double *liveL);

/* The data sets still running (multi_nested_sampler.py:148-173): rows int32[nrun], ascending
 * original indices.  prepare/advance work on exactly these, in this order. */
int mdns_joint_set_running(mdns_joint *j, const int *rows, int nrun);

/* Start of an iteration (multi_nested_sampler.py:130-143 `prepare`): per running data set the
 * lowest live likelihood Lmin f64[nrun] and its live slot argmin int32[nrun] (first occurrence,
 * as numpy.argmin); shelf entries that no longer beat Lmin are dropped in order (:137-138) --
 * keep uint64[nrun * ceil(cap/64)] gets, per data set, bit k of word k/64 set when its entry k
 * stays (words per data set: mdns_joint_keep_words); thresholds are refreshed. */
int mdns_joint_prepare(mdns_joint *j, double *Lmin, int *argmin, unsigned long long *keep);
int mdns_joint_keep_words(const mdns_joint *j);
/* End of an iteration (multi_nested_sampler.py:494-534): every running data set gives up the
 * live point found by the last prepare and takes the head of its shelf.  Fails when a running
 * data set has an empty shelf. */
int mdns_joint_advance(mdns_joint *j);
/* Make room for shelves of at least `shelf_cap` entries (contents kept). */
int mdns_joint_reserve(mdns_joint *j, int shelf_cap);
int mdns_joint_shelf_cap(const mdns_joint *j);

/*
 * One chunk of a constrained draw (hiermetriclearn.py:181-196 + multi_nested_sampler.py:462-485):
 * the B candidates params f64[B,3] (already proposed by the host, in order) are scored against
 * the M selected spectra row_ids int32[M] (ascending original indices; NULL = all, M = ndata);
 * candidate b is acceptable when it beats the threshold of at least one selected data set
 * (`any(L > Lmins)`, hiermetriclearn.py:193).  *accepted = index of the FIRST acceptable
 * candidate, or -1.  For that candidate only: Lrow f64[M] its likelihoods, fillbits
 * uint64[ceil(M/64)] with bit k set when it beats the threshold of the k-th selected data set
 * (multi_nested_sampler.py:482-485); those data sets' shelves receive it and their thresholds
 * move up, all on the device.  Likelihoods of the other candidates never reach memory.
 * Lrow may be NULL (the row then stays on the device).  B <= 1024.
 */
int mdns_joint_draw_gauss(mdns_joint *j, const double *params, int B, double noise_level,
                          const int *row_ids, int M, int *accepted, double *Lrow,
                          unsigned long long *fillbits);
#define MDNS_JOINT_MAX_BATCH 1024
/* The two halves of that call for hosts that put something between them: `score` stages the
 * candidates and leaves one accept flag per candidate on the device (mdns_joint_flags_dev); with
 * the data sets sharded over several GPUs the ranks MAX-reduce those flags; `commit` then takes
 * the first flagged candidate and returns its index, likelihood row and fill bits for the
 * selection given to `score`. */
int mdns_joint_score(mdns_joint *j, const double *params, int B, double noise_level,
                     const int *row_ids, int M);
int mdns_joint_commit(mdns_joint *j, int *accepted, double *Lrow, unsigned long long *fillbits);

/* Current thresholds of all data sets, higher f64[ndata] (tests; NaN before the first prepare),
 * and the shelf sizes n int32[ndata]. */
int mdns_joint_get_thresholds(mdns_joint *j, double *higher, int *shelf_n);

/* ------------------------------------------------------------------------------------ */
/* Part 3: raw device entry points (all pointers are DEVICE pointers; asynchronous on the */
/* library stream; no host synchronisation)                                             */
/* ------------------------------------------------------------------------------------ */

void *mdns_dev_alloc(size_t bytes);
void mdns_dev_free(void *p);
int mdns_h2d(void *dst, const void *src, size_t bytes);   /* synchronous */
int mdns_d2h(void *dst, const void *src, size_t bytes);   /* synchronous */
int mdns_d2d(void *dst, const void *src, size_t bytes);   /* asynchronous, library stream */
int mdns_sync(void);                                      /* wait for the library stream */
/* Run on a caller-owned hipStream_t (e.g. the stream of an RCCL collective); NULL restores
 * the library's own stream. */
int mdns_set_stream(void *hip_stream);

/* HIP events on the library stream (bench.py times launches with these). */
void *mdns_event_create(void);
void mdns_event_destroy(void *ev);
int mdns_event_record(void *ev);
double mdns_event_elapsed_ms(void *ev_start, void *ev_stop);   /* synchronises on ev_stop */

/* Per-launch timing of the dominant kernels with HIP events on the library stream.
 * Kernel classes: 0 = gauss log-likelihood, 1 = muse log-likelihood, 2 = count-within,
 * 3 = bootstrap nearest-chosen.  mdns_profile(classes) takes a bit mask (bit k = class k; 15 =
 * all): it clears the statistics of the named classes and records from now on exactly those;
 * mdns_profile(0) stops.  Every timed launch costs two event records on the stream (about
 * 9 us per 90 us step of bench.py when every launch is timed), so time only what is being
 * measured; mdns_profile_every(n) times every n-th launch of a class only (default 1).
 * mdns_profile_read synchronises and returns, for kernel class `which`, the number of launches
 * timed and the sum of their durations in milliseconds.  mdns_profile_kernel names the
 * kernel instantiation last launched for that class (as rocprofv3 prints it, without the
 * namespace), e.g. "k_gauss_cols<8, 1>". */
int mdns_profile(int classes);
int mdns_profile_every(int n);
int mdns_profile_read(int which, long long *launches, double *total_ms);
const char *mdns_profile_kernel(int which);

/* d_params f64[B,3], d_row_ids int32[M] or NULL, d_Lout f64[B,M]. */
int mdns_gauss_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                 double noise_level, const int *d_row_ids, int M,
                                 double *d_Lout);
int mdns_muse_loglike_batch_dev(mdns_spectra *s, const double *d_ypred, int B,
                                const int *d_row_ids, int M, double *d_Lout);
int mdns_muse3_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                 const int *d_row_ids, int M, double *d_Lout);
/* d_params f64[B, mdns_spectra_nparams(s)]: the handle's line list, or the built-in model without one. */
int mdns_lines_loglike_batch_dev(mdns_spectra *s, const double *d_params, int B,
                                 const int *d_row_ids, int M, double *d_Lout);

/* d_curves f64[B] rows of ldc >= nx doubles, d_row_ids int32[M] or NULL, d_Lout f64[B][M]. */
int mdns_curve_loglike_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, double noise_level,
                                 const int *d_row_ids, int M, double *d_Lout);

/* The two halves of mdns_joint_draw_gauss on device pointers, nothing waits for the host:
 * score leaves one accept flag per candidate in the handle (int32[MDNS_JOINT_MAX_BATCH], 1 =
 * beats some selected data set of THIS handle's spectra; mdns_joint_flags_dev -- with the data
 * sets sharded over ranks a MAX all-reduce of that buffer in place makes every rank see every
 * rank's flags), commit takes the first flagged candidate and leaves, in the handle's result
 * buffer (mdns_joint_result_dev; device memory, valid until the next score),
 * {int32 accepted, int32 status (0 ok, 1 shelf overflow), 8 bytes unused} | fillbits
 * uint64[ceil(M/64)] | Lrow f64[M]  (mdns_joint_result_bytes(M) bytes in all). */
int mdns_joint_score_dev(mdns_joint *j, const double *d_params, int B, double noise_level,
                         const int *d_row_ids, int M);
int *mdns_joint_flags_dev(mdns_joint *j);
int mdns_joint_commit_dev(mdns_joint *j, const int *d_row_ids, int M);
/* The same without the likelihood row (Lrow in the result buffer is left as it was): who beats its
 * threshold and with which likelihood is taken from what the score pass kept of the candidates it
 * flagged, nothing is computed again.  This is what mdns_joint_draw_gauss / mdns_joint_commit do
 * when called with Lrow == NULL. */
int mdns_joint_commit_bits_dev(mdns_joint *j, const int *d_row_ids, int M);
const void *mdns_joint_result_dev(mdns_joint *j);
size_t mdns_joint_result_bytes(int M);
/* The outcome of the last mdns_joint_commit_dev without a copy: a kernel behind the commit pass
 * leaves {accepted, status, fill words} in host memory mapped into the device, `seq` last; this call
 * polls for it (no stream synchronisation) and hands over *accepted and, when a candidate was
 * accepted, fillbits uint64[ceil(M/64)] (may be NULL).  M as passed to the commit. */
int mdns_joint_fetch(mdns_joint *j, int M, int *accepted, unsigned long long *fillbits);
/* prepare / advance without the copies to the host (results stay in the handle);
 * mdns_joint_restore_live_dev overwrites the live matrix from d_liveL f64[nlive, ndata] and
 * empties the shelves (bench.py re-runs the same iteration). */
int mdns_joint_prepare_dev(mdns_joint *j);
int mdns_joint_advance_dev(mdns_joint *j);
int mdns_joint_restore_live_dev(mdns_joint *j, const double *d_liveL);
/* Takes back the last mdns_joint_advance[_dev]: every running data set's replaced live slot gets
 * the likelihood back that the preceding prepare found there; shelves emptied (bench.py). */
int mdns_joint_undo_advance_dev(mdns_joint *j);
/* The live matrix f64[nlive, ndata] where it lies, to read: the entries above are its only writers (a commit trusts what
 * the last prepare saw of a column until one of them, or the next prepare, says otherwise). */
const double *mdns_joint_live_dev(mdns_joint *j);

/* K3 on device: d_members f64[K,ndim], d_cands f64[M,ndim]; d_counts int32[M] is
 * OVERWRITTEN with the number of members strictly within maxdistance (no early stop). */
int mdns_count_within_dev(const double *d_members, int K, int ndim, double maxdistance,
                          const double *d_cands, int M, int *d_counts);
/* K6 on device: d_chosen f64[K,nbootstraps]; d_round_sq f64[nbootstraps] receives, per round,
 * max over left-out points i>=1 of the squared distance to the nearest chosen point
 * (radius = sqrt of the max over rounds). */
int mdns_bootstrap_round_maxsq_dev(const double *d_members, int K, int ndim,
                                   const double *d_chosen, int nbootstraps,
                                   double *d_round_sq);

/* ------------------------------------------------------------------------------------------
 * Part 4 -- grouping of the data sets that share live points.
 *
 * Replaces, behind `MultiNestedSampler.generate_subsets_graph` (multi_nested_sampler.py:268-355),
 * igraph's `Graph.clusters()` on the bipartite graph {data sets} -- {live points} (:319-325)
 * and the `numpy.unique(live_pointsp[:, selected])` in front of it (:279): connected components
 * by minimum-label propagation on the device, the distinct ids as a bit map.  Integer results,
 * independent of the order the hardware works in.
 *
 * The handle keeps the id matrix `live_pointsp` (int32[nlive][ndata], C order, :108) on the
 * device, indexed by the ORIGINAL data-set index for the whole run.
 * ------------------------------------------------------------------------------------------ */
typedef struct mdns_groups mdns_groups;
mdns_groups *mdns_groups_create(int nlive, int ndata);
void mdns_groups_destroy(mdns_groups *g);
/* the whole matrix, ids int32[nlive][ndata] */
int mdns_groups_set_ids(mdns_groups *g, const int32_t *ids);
int mdns_groups_get_ids(mdns_groups *g, int32_t *ids);
/* End of an iteration (multi_nested_sampler.py:510-520): data set rows[i] gives up the live point
 * in slot slots[i] and takes new_ids[i]; n entries, rows distinct. */
int mdns_groups_replace(mdns_groups *g, const int32_t *rows, const int32_t *slots,
                        const int32_t *new_ids, int n);
/* Connected components over the data sets rows[0..M) (ascending original indices; NULL with
 * M == ndata: all).  Every id must lie in [0, npoints).  *ncomponents receives their number,
 * *ndistinct the number of distinct ids the selection holds and `distinct` (int32[cap], may be
 * NULL) those ids in ascending order -- numpy.unique of the selected columns (:279).  `touched`
 * (uint64[ceil(npoints/64)], may be NULL) receives the same set as a bit map: bit q = some
 * selected data set holds live point q. */
int mdns_groups_components(mdns_groups *g, const int32_t *rows, int M, long long npoints,
                           int *ncomponents, long long *ndistinct, int32_t *distinct, long long cap,
                           unsigned long long *touched);
/* Of the last mdns_groups_components: labels int32[M] = the lowest data-set index of the
 * component rows[i] lies in (components in ascending label order are igraph's cluster order,
 * which numbers them by their first vertex); point_labels int32[npoints] = the label of the
 * component holding live point q, -1 when no selected data set holds it.  Either may be NULL.
 * "Last" means the last call that SUCCEEDED with nothing after it: a components call that fails (an id
 * out of range, the deferred bit of a bad mdns_groups_replace, `cap` too small, refused arguments), like
 * a change of the ids, leaves this call and mdns_groups_id_labels refused until the next success. */
int mdns_groups_labels(mdns_groups *g, int32_t *labels, int32_t *point_labels);
/* The same for the ids the last mdns_groups_components listed only: id_labels int32[ndistinct], in the
 * order of that list (a full mdns_groups_labels copies one label per id of the PILE, megabytes late in
 * a run, of which the caller looks at the listed ones). */
int mdns_groups_id_labels(mdns_groups *g, int32_t *labels, int32_t *id_labels, long long ndistinct);
/* rounds of label propagation per mdns_groups_components call so far, on average */
double mdns_groups_mean_rounds(const mdns_groups *g);

/* ------------------------------------------------------------------------------------------
 * Part 5 -- one native call per constrained draw (libmdns_host.so, csrc/host_constrainer.cpp).
 *
 * The reference's MLFriends constrainer (hiermetriclearn.py:27-211 over
 * clustering/radfriendsregion.py:58-182 and clustering/sdml.py:60-88) as ONE object behind the C
 * ABI: rebuild policy (:152-166,198-211), region construction with its bootstrap draws
 * (:48-92; neighbors.py:170-177), the candidate generators (radfriendsregion.py:117-182,
 * hiermetriclearn.py:104-137) and the accept loop (:181-196).  Every random number is taken from
 * numpy's OWN Mersenne-Twister state (the address the caller passes: `mt19937_state` behind
 * numpy.random's global legacy RandomState), with numpy's legacy algorithms, in the reference's
 * call order -- the stream advances exactly as if the reference had run.  The kernels are reached
 * through a table of C function pointers: on the GPU the mdns_backend_* entry points of
 * libmdns_hip.so below; tests put the CPU oracle behind the same table.
 * ------------------------------------------------------------------------------------------ */
#define MDNS_MAX_DIM 16

struct mdns_chain_request;
/* Device work of a draw.  `user` is passed back as the first argument of every function. */
typedef struct mdns_draw_backend {
	void *user;
	/* RadFriendsRegion(members, maxdistance) (radfriendsregion.py:59-70): members f64[K, ndim] in
	 * the metric's coordinates.  packed != NULL: K6 with that bootstrap choice (bit b of packed[i] =
	 * point i chosen in round b; cneighbors.c:125-179), *radius receives the result; packed == NULL:
	 * the region gets the radius *radius holds.  Returns an opaque region, NULL on failure. */
	void *(*region_create)(void *user, const double *members, int K, int ndim,
	                       const unsigned *packed, int nbootstraps, double *radius);
	void (*region_destroy)(void *user, void *region);
	/* K3 with the region's radius (cneighbors.c:95-119, no early stop): counts int32[n]. */
	int (*region_count)(void *user, void *region, const double *points, int n, int *counts);
	/* A constrained draw over the data sets rows int32[M] (ascending ORIGINAL indices; NULL: all,
	 * M = their number) begins: called once before its chunks. */
	int (*draw_begin)(void *user, const int *rows, int M);
	/* One chunk: params f64[B, nparams] of ALREADY proposed candidates, in order.  *accepted = the
	 * first that beats the threshold of some selected data set (hiermetriclearn.py:193), or -1;
	 * fillbits uint64[ceil(M/64)]: bit k set when it beats the k-th selected data set's
	 * (multi_nested_sampler.py:482-485); those data sets take the point in.  *nscored = candidates
	 * looked at (B, or fewer when the scorer stops at the accepted one).  jitter (NULL, or f64[B, M]):
	 * added to the likelihoods before they are compared and kept (musefuse.py:535). */
	int (*draw_chunk)(void *user, const double *params, int B, const double *jitter, int *accepted,
	                  unsigned long long *fillbits, int *nscored);
	/* How many of `offered` candidates one chunk should hold for M selected data sets when the last
	 * draw of this constrainer needed `hint` tries (a speed choice: results do not depend on it). */
	int (*chunk_size)(void *user, int offered, int M, int hint);
	/* Optional (NULL: region_create is used).  region_create with packed != NULL in two halves, so
	 * that the caller can work while K6 runs: region_begin uploads the members and launches K6 and
	 * returns the region at once, region_radius waits for the radius of such a region.  At most one
	 * region per backend is between the two calls at any time. */
	void *(*region_begin)(void *user, const double *members, int K, int ndim, const unsigned *packed, int nbootstraps);
	int (*region_radius)(void *user, void *region, double *radius);
	/* Optional (NULL: not offered).  The first batch of box proposals of a region between region_begin
	 * and region_radius WITHOUT a host look in between (radfriendsregion.py:135-141 + hiermetriclearn.py:
	 * 111-119,181-196): chain_begin queues, behind K6, the proposals lo + (hi - lo) u, their membership
	 * counts and -- when it can; limit > 0 asks for it -- the first chunk of the draw begun with
	 * draw_begin: the first min(kept, limit) proposals that are inside the region and, after the metric's
	 * inverse transform, inside the unit cube, prior-transformed, scored, accepted and committed like a
	 * draw_chunk.  chain_end waits for all of it: counts int32[n]; *nkept (-1: the chunk did not ride
	 * along), *B (its size), *accepted, fillbits, params f64[B][nparams] the device scored with (may be
	 * NULL).  The caller then asks region_radius as usual. */
	/* Optional (NULL: not offered): the likelihood noise in BAND form (musefuse.py:535 without one
	 * deviate per evaluation).  draw_band scores the chunk like draw_chunk, WITHOUT noise, and compares
	 * every likelihood with its threshold +- 1.01 bound[b] (bound f64[B]: no deviate of candidate b exceeds
	 * it): status int32[B] = 1 when some selected data set is beaten whatever the noise, 0 when none can
	 * be, 2 when that hangs on the pairs listed: pair_b / pair_k int32 (candidate, position in the
	 * selection), pair_L / pair_thr f64 (likelihood without noise, threshold); *npairs their number.  The
	 * arrays hold cap entries and the device keeps at most 4096 pairs of a chunk: with no more pairs than
	 * min(cap, 4096) *npairs is their true number and all of them are handed over; with more, the first
	 * min(cap, 4096) are and *npairs > cap (the caller falls back to draw_chunk with the whole block).
	 * Nothing is committed.
	 * draw_band_commit: candidate b is the accepted one; jitter_row f64[M] is added to its likelihoods,
	 * then shelves, thresholds and fill bits as in draw_chunk. */
	int (*draw_band)(void *user, const double *params, int B, const double *bound, int *status, int *npairs,
	                 int *pair_b, int *pair_k, double *pair_L, double *pair_thr, int cap);
	int (*draw_band_commit)(void *user, int b, const double *jitter_row, unsigned long long *fillbits);
	int (*chain_begin)(void *user, void *region, const struct mdns_chain_request *rq);
	int (*chain_end)(void *user, void *region, int *counts, int *nkept, int *B, int *accepted,
	                 unsigned long long *fillbits, double *params);
	/* Optional (all three or none): draw_band in two halves with a cheap look in between.  While a chunk
	 * is being scored the constrainer already advances the stream for the candidates that FOLLOW it in
	 * the same batch (their bounds do not depend on the outcome; if the chunk accepts somebody that work is
	 * dropped), one candidate at a time until draw_band_ready returns nonzero. */
	int (*draw_band_begin)(void *user, const double *params, int B, const double *bound);
	int (*draw_band_ready)(void *user);
	int (*draw_band_end)(void *user, int *status, int *npairs, int *pair_b, int *pair_k, double *pair_L, double *pair_thr, int cap);
} mdns_draw_backend;

struct mdns_prior;
typedef struct mdns_chain_request {
	int n, ndim;                    /* proposals, dimensions */
	const double *u;                /* f64[n][ndim]: numpy's raw doubles of uniform(lo, hi, size=(n, ndim)) */
	const double *mn, *mx;          /* f64[ndim]: members.min(axis=0), members.max(axis=0) (radfriendsregion.py:69-70) */
	int identity;                   /* the metric is the identity; else x = y * scale + mean (sdml.py) */
	const double *mean, *scale;
	const struct mdns_prior *prior;
	int limit;                      /* candidates of the first chunk at most; 0: stop after the counts */
} mdns_chain_request;

/* The prior transform of the problem (sample.py:52-58) and the kernel's parameters (sample.py:103),
 * per dimension:  x[k] = a[k] * u[k] + b[k]  (the addition skipped when b[k] == 0), then
 * x[k] = 10 ** x[k] where pow10[k];  kernel parameter k = x[k], or 10 ** x[k] where
 * kernel_pow10[k].  `custom`, when set, replaces all of that: it fills x f64[B, ndim] and
 * params f64[B, nparams] from u f64[B, ndim] (a problem definition kept in Python). */
typedef struct mdns_prior {
	int ndim, nparams;
	double a[MDNS_MAX_DIM], b[MDNS_MAX_DIM];
	int pow10[MDNS_MAX_DIM], kernel_pow10[MDNS_MAX_DIM];
	void (*custom)(void *user, const double *u, int B, double *x, double *params);
	void *user;
	/* > 0: every likelihood evaluation adds N(0, jitter_sigma) noise per selected data set, drawn from
	 * the global stream in evaluation order -- `Lout[data_mask] + numpy.random.normal(0, 1e-5,
	 * size=data_mask.sum())`, musefuse.py:535.  The constrainer draws the deviates of a chunk's
	 * candidates one candidate after the other and, when one is accepted, puts the stream back to where
	 * it stood after THAT candidate's deviates (the reference never evaluates the ones behind it). */
	double jitter_sigma;
} mdns_prior;

/* numpy operations the constrainer leaves to numpy itself so that its numbers ARE numpy's (numpy
 * dispatches power/log2 to SIMD code whose last bits differ from the C library's):
 * vec_pow: inout[i] = numpy.power(inout[i], exponent)  (radfriendsregion.py:156);
 * fit_metric: mean f64[ndim], scale f64[ndim] of sdml.py:44-49 (kind 1) / :68-82 (kind 2) fitted to
 * u f64[K, ndim] shifted to its mean (hiermetriclearn.py:63-80); returns 0. */
typedef struct mdns_numpy_ops {
	void *user;
	void (*vec_pow)(void *user, double *inout, int n, double exponent);
	int (*fit_metric)(void *user, int kind, const double *u, int K, int ndim, double *mean, double *scale);
} mdns_numpy_ops;

typedef struct mdns_constrainer mdns_constrainer;

#define MDNS_METRIC_NONE 0
#define MDNS_METRIC_SIMPLESCALING 1
#define MDNS_METRIC_TRUNCATEDSCALING 2

/* MetricLearningFriendsConstrainer(metriclearner, rebuild_every, metric_rebuild_every,
 * force_shrink) (hiermetriclearn.py:28-46). */
mdns_constrainer *mdns_constrainer_create(int ndim, int metriclearner, int rebuild_every,
                                          int metric_rebuild_every, int force_shrink);
void mdns_constrainer_destroy(mdns_constrainer *c, const mdns_draw_backend *be);
/* `constrainer.region = None` (cachedconstrainer.py:104-105): the next draw builds a new region. */
void mdns_constrainer_forget_region(mdns_constrainer *c);

/* draw_constrained (hiermetriclearn.py:173-211).  live points: rows `ids` (int32 or int64 by
 * ids_itemsize, K of them, in the caller's order) of pile_u f64[npile, ndim]; selection rows/M as in
 * mdns_draw_backend.draw_begin.  Out: u f64[ndim] the accepted unit-cube point, x f64[ndim] its
 * prior transform, *ntries the likelihood calls the reference would have made (its `ntoaccept`),
 * fillbits uint64[ceil(M/64)].  Returns 0; on failure non-zero and mdns_host_last_error(). */
int mdns_constrainer_draw(mdns_constrainer *c, const mdns_draw_backend *be, const mdns_prior *prior,
                          const mdns_numpy_ops *np, void *mt19937_state,
                          const double *pile_u, const void *ids, int ids_itemsize, int K,
                          const int *rows, int M,
                          double *u, double *x, long long *ntries, unsigned long long *fillbits);
/* counters since creation, out int64[MDNS_CONSTRAINER_COUNTERS]: [0] draws, [1] chunks, [2] candidates
 * scored, [3] (candidate, data set) pairs scored, [4] regions built, [5] radius computations (K6),
 * [6] membership calls (K3), [7] raw proposals, [8] proposals the region kept, [9] tries (the
 * reference's likelihood calls); nanoseconds spent in [10] the bootstrap choices, [11] region_create
 * (K6 + upload), [12] region_count (K3), [13] proposal random numbers + arithmetic, [14] the prior
 * transform, [15] draw_chunk, [16] mdns_constrainer_draw as a whole, [17] the likelihood jitter;
 * [18] first batches chained on the device together with their chunk (chain_begin / chain_end), [19] with
 * their membership counts only, [20] accepted candidates of chained chunks whose device parameters were
 * not bit for bit the host's (10**v), [21] nanoseconds between chain_begin and chain_end; [22] pairs the
 * device could not decide without their noise (draw_band), [23] candidates whose noise was replayed for them,
 * [24] candidates whose bound was ready before their chunk (made while the previous chunk was scored).
 * mdns_constrainer_share_stats:
 * every increment is also added to totals int64[MDNS_CONSTRAINER_COUNTERS] (the caller's: the sum
 * over a sampler's constrainers). */
#define MDNS_CONSTRAINER_COUNTERS 25
void mdns_constrainer_stats(const mdns_constrainer *c, long long *out);
void mdns_constrainer_share_stats(mdns_constrainer *c, long long *totals);
const char *mdns_host_last_error(void);
/* The cached second deviate of numpy's legacy Gaussian generator (legacy-distributions.c,
 * `has_gauss` / `gauss`): the constrainer keeps it for the process like numpy's global RandomState
 * does; callers that mix their own numpy.random.normal calls with native draws hand it over. */
void mdns_host_rng_get_gauss(int *has_gauss, double *gauss);
void mdns_host_rng_set_gauss(int has_gauss, double gauss);

/* The backend of a Gaussian-line joint state on the GPU (libmdns_hip.so): the functions to put
 * into mdns_draw_backend, user = the mdns_joint handle.  region_create = K6 + resident members
 * (mdns_region_create_bootstrapped / mdns_region_create + mdns_region_set_radius), region_count =
 * mdns_region_count, draw_chunk = mdns_joint_draw_gauss without the likelihood row. */
void *mdns_backend_region_create(void *joint, const double *members, int K, int ndim,
                                 const unsigned *packed, int nbootstraps, double *radius);
void mdns_backend_region_destroy(void *joint, void *region);
int mdns_backend_region_count(void *joint, void *region, const double *points, int n, int *counts);
int mdns_backend_draw_begin(void *joint, const int *rows, int M);
int mdns_backend_draw_chunk(void *joint, const double *params, int B, const double *jitter, int *accepted,
                            unsigned long long *fillbits, int *nscored);
int mdns_backend_chunk_size(void *joint, int offered, int M, int hint);
void *mdns_backend_region_begin(void *joint, const double *members, int K, int ndim, const unsigned *packed, int nbootstraps);
int mdns_backend_region_radius(void *joint, void *region, double *radius);
/* mdns_backend_draw_chunk for a model the CALLER evaluates: curves f64[B][nx], one model curve per candidate, in
 * place of the parameter rows (after mdns_backend_draw_begin; same outputs; jitter NULL or f64[B][M]; a state
 * of any statistic).  Scored as mdns_curve_loglike_batch at the noise level of mdns_joint_init_curves / _init_gauss (no
 * variances), as mdns_muse_loglike_batch (variances), as mdns_curve_chi2_batch (variances, fixed scale: Part 9) or as
 * mdns_curve_poisson_batch (counts: Part 10; with a background mdns_curve_wstat_batch: Part 11), decided and committed
 * like a draw_chunk.  A draw may mix
 * parameter chunks and curve chunks.  _dev: curves (rows of ldc >= nx doubles) and jitter already in device memory,
 * read on the library stream. */
int mdns_backend_draw_curves(void *joint, const double *curves, int B, const double *jitter, int *accepted,
                             unsigned long long *fillbits, int *nscored);
int mdns_backend_draw_curves_dev(void *joint, const double *d_curves, int ldc, int B, const double *d_jitter, int *accepted,
                                 unsigned long long *fillbits, int *nscored);
/* mdns_backend_draw_chunk in two halves, for hosts that put something between them -- with the data sets
 * sharded over ranks a MAX all-reduce of the candidates' votes: `score` (after draw_begin)
 * stages and scores the chunk like draw_chunk and leaves one int32 0 / 1 vote per candidate in device
 * memory (mdns_joint_votes_dev: int32[MDNS_JOINT_MAX_BATCH], asynchronous on the library stream);
 * `commit` takes the first candidate that has a vote THEN as the accepted one and finishes like
 * draw_chunk (shelves, thresholds, *accepted, fill bits of this handle's selected data sets).  The two
 * statistics with a parameter model (Gaussian line; scale-marginalised likelihood with jitter f64[B, M]). */
int mdns_backend_draw_score(void *joint, const double *params, int B, const double *jitter);
int *mdns_joint_votes_dev(mdns_joint *j);
int mdns_backend_draw_commit(void *joint, int *accepted, unsigned long long *fillbits);
/* the HIP stream the library launches on (its own, or the one given to mdns_set_stream) */
void *mdns_get_stream(void);
int mdns_backend_draw_band(void *joint, const double *params, int B, const double *bound, int *status, int *npairs,
                           int *pair_b, int *pair_k, double *pair_L, double *pair_thr, int cap);
int mdns_backend_draw_band_commit(void *joint, int b, const double *jitter_row, unsigned long long *fillbits);
int mdns_backend_draw_band_begin(void *joint, const double *params, int B, const double *bound);
int mdns_backend_draw_band_ready(void *joint);
int mdns_backend_draw_band_end(void *joint, int *status, int *npairs, int *pair_b, int *pair_k, double *pair_L, double *pair_thr, int cap);
/* mdns_backend_draw_band scores large chunks (>= 8 candidates x >= 512 spectra) as two matrix products on
 * v_mfma_f64_16x16x4_f64 with the band widened by a rigorous bound on the rounding of that form
 * (csrc/mdns_k2gemm.hip); whatever that leaves undecided is scored again by the exact row kernels, and the
 * accepted candidate's row always is.  mode: -1 by shape (default; MDNS_K2_FILTER=0 / 1 at start), 0 never,
 * 1 for every chunk.  stats: chunks filtered | of those scored again exactly | exact rows made for a
 * commit | spectra handles prepared. */
void mdns_muse_filter_mode(int mode);
/* the filter pass alone on device pointers (asynchronous on the library stream): d_ypred f64[B][nx] templates,
 * d_thr f64[ndata] thresholds by data set, d_bound f64[B]; d_out int32[2 B + 1], zeroed by the caller: [b] set to
 * 1 when candidate b certainly beats a threshold, [B + b] when a pair of its cannot be settled, [2 B] the number
 * of such pairs */
int mdns_muse_filter_dev(mdns_spectra *s, const double *d_ypred, int B, const int *d_row_ids, int M, const double *d_thr,
                         const double *d_bound, int *d_out);
void mdns_muse_filter_stats(long long *out4);
int mdns_backend_chain_begin(void *joint, void *region, const mdns_chain_request *rq);
int mdns_backend_chain_end(void *joint, void *region, int *counts, int *nkept, int *B, int *accepted,
                           unsigned long long *fillbits, double *params);

/* ------------------------------------------------------------------------------------------
 * Part 6 -- one native call per nested-sampling ITERATION (libmdns_host.so, csrc/host_sampler.cpp).
 *
 * The integer side of MultiNestedSampler between `prepare` and the replacement of the dead points
 * (multi_nested_sampler.py:365-534): the passes over the data sets whose shelf is empty, the grouping
 * of the data sets that share live points (:204-355), the constrainer that serves each group
 * (cachedconstrainer.py:19-116: four-generation cache, "similar to the last call" shortcut, one
 * constrainer per single data set), the constrained draws (mdns_constrainer_draw) and the shelves'
 * queues of point ids (:474-489), the pile of accepted points, the superpoints.  The floating-point
 * side stays where it is: the joint state behind `mdns_draw_backend`.  Python keeps the reference's
 * class (massivedatans_amd.core.NativeCoreSampler: same constructor, iterator protocol, attributes).
 * ------------------------------------------------------------------------------------------ */
/* Connected components of big selections on the device: user = an mdns_groups handle, the three
 * functions = mdns_groups_components / mdns_groups_id_labels / mdns_groups_replace (Part 4).  Optional:
 * without it (and for selections of few (data set, live point) pairs) a union-find on the host gives
 * the same partition, component order and ascending id lists. */
typedef struct mdns_group_backend {
	void *user;
	int (*components)(void *user, const int32_t *rows, int M, long long npoints, int *ncomponents,
	                  long long *ndistinct, int32_t *distinct, long long cap, unsigned long long *touched);
	int (*id_labels)(void *user, int32_t *labels, int32_t *id_labels, long long ndistinct);
	int (*replace)(void *user, const int32_t *rows, const int32_t *slots, const int32_t *new_ids, int n);
} mdns_group_backend;

typedef struct mdns_core mdns_core;

/* MultiNestedSampler(...) (multi_nested_sampler.py:58-119) with the constrainer settings of the
 * reference's driver (sample.py:133-137).  be / prior / np / mt19937_state as in mdns_constrainer_draw
 * (borrowed for the life of the object); gb may be NULL; shelf_mirror (int64[ndata], may be NULL) is
 * incremented at the ORIGINAL index of every data set that shelves a point (the joint state's mirror of
 * its shelf sizes; the joint state itself takes entries off in its `advance`); constrainer_totals as in
 * mdns_constrainer_share_stats (may be NULL). */
mdns_core *mdns_core_create(int nlive, int ndata, int ndim, int nsuperset_draws, int use_graph,
                            int metriclearner, int rebuild_every, int metric_rebuild_every, int force_shrink,
                            const mdns_draw_backend *be, const mdns_prior *prior, const mdns_numpy_ops *np,
                            void *mt19937_state, const mdns_group_backend *gb, long long *shelf_mirror,
                            long long *constrainer_totals);
void mdns_core_destroy(mdns_core *c);
const char *mdns_core_last_error(void);
/* selections of at most this many (data set, live point) pairs are grouped on the host even when a
 * device backend is there (default 32768) */
void mdns_core_set_host_edges(mdns_core *c, long long edges);
/* The focussed passes of an iteration select ever fewer data sets: their components are analysed once
 * per iteration (selections of at most edges_max pairs; 0: never) and then kept up to date as data sets
 * leave (csrc/host_sampler_inc.h); check != 0 compares every such result with a fresh computation. */
void mdns_core_set_incremental(mdns_core *c, long long edges_max, int check);
/* the nlive prior draws every data set starts from (:88-103): u, x f64[nlive][ndim] */
int mdns_core_set_initial(mdns_core *c, const double *u, const double *x);
/* `prepare` (:137-138): keep uint8[nrunning][width]; entry e of the r-th running data set's shelf stays
 * when e < width and keep[r][e] */
int mdns_core_purge(mdns_core *c, const unsigned char *keep, int width);
/* :365-491: constrained draws until no running data set has an empty shelf */
int mdns_core_fill(mdns_core *c);
/* :494-534: the r-th running data set gives up the live point in slot argmin[r] and takes the head of
 * its shelf; dead_u, dead_x f64[nrunning][ndim] / dead_ids, new_ids int32[nrunning] may be NULL */
int mdns_core_advance(mdns_core *c, const int32_t *argmin, double *dead_u, double *dead_x,
                      int32_t *dead_ids, int32_t *new_ids);
/* cut_down (:148-173): surviving uint8[nrunning] */
int mdns_core_cut_down(mdns_core *c, const unsigned char *surviving);
long long mdns_core_npoints(const mdns_core *c);
int mdns_core_nrunning(const mdns_core *c);
/* the pile of accepted points f64[npoints][ndim] (valid until the next mdns_core_fill) */
const double *mdns_core_pile_u(const mdns_core *c);
const double *mdns_core_pile_x(const mdns_core *c);
/* live_pointsp int32[nlive][nrunning] (:108) */
int mdns_core_get_ids(const mdns_core *c, int32_t *out);
/* shelf sizes int32[nrunning] and (ids != NULL) the waiting ids, queue after queue; returns their number */
long long mdns_core_get_shelves(const mdns_core *c, int32_t *sizes, int32_t *ids, long long cap);
int mdns_core_get_superpoints(const mdns_core *c, int32_t *out, int cap);
/* out int64[MDNS_CORE_COUNTERS]: [0] ndraws (likelihood calls of the reference), [1] constrained draws,
 * [2] useful (candidate, data set) evaluations, [3] points in the pile, [4] iterations, [5] running data
 * sets, [6] superpoints, [7] passes, [8] groupings, of which [9] on the host, [10] on the device, [11] walks,
 * [12] constrainers created, nanoseconds in [13] mdns_constrainer_draw, [14] grouping, [15] mdns_core_fill,
 * [16] draws served by the "similar to the last call" shortcut, [17..24] groupings by selection size
 * (fewer than 2, 8, 32, 128, 512, 2048, 8192 data sets, more) and [25..32] the nanoseconds they took;
 * focussed groupings kept up to date: [33] analyses from scratch, [34] updates, [35] updates that split a component */
#define MDNS_CORE_COUNTERS 36
void mdns_core_stats(const mdns_core *c, long long *out);

/* ------------------------------------------------------------------------------------------
 * Part 7 -- posterior summaries and resampling of finished runs (csrc/mdns_posterior.hip).
 *
 * Replaces the reference's per-spectrum post-processing loop (musefuse_postprocess.py:112-140,
 * checkoutput.py:27-44).  Input: what save_results writes, host arrays in C order,
 * w, L double[nsamp][ndata] and x double[nsamp][ndata][ndim] (1 <= ndim <= 8); they are uploaded
 * once and serve every call on the handle.  Per data set d, with lw = w + L and F its rows where lw
 * is finite, p = exp(lw[F] - max) / sum:
 *   nfinite[d] = |F|, log_norm[d] = max + log(sum), ess[d] = 1 / sum p^2 (Kish),
 *   mean / std [ndata][ndim]: the exact weighted moments (std: centred second pass),
 *   quant [ndata][ndim][nq]: for each q[j] in (0, 1], the smallest sample value whose cumulative
 *     weight in value order reaches q[j] (a sample value; weights in 2^-52 fixed point),
 *   imaxL[d]: the row of F with the largest L (the first on ties).
 * A data set with nfinite = 0 gets NaN statistics, imaxL = -1 and draws of -1.  Every output is
 * optional (NULL: not fetched; std and quant are not computed either).  No float atomics: the
 * same input gives the same bytes.  0 on success, message in mdns_last_error().
 * ------------------------------------------------------------------------------------------ */
typedef struct mdns_posterior mdns_posterior;
mdns_posterior *mdns_posterior_create(const double *w, const double *L, const double *x,
                                      int nsamp, int ndata, int ndim);
void mdns_posterior_destroy(mdns_posterior *h);
int mdns_posterior_summary(mdns_posterior *h, const double *q, int nq, int *nfinite,
                           double *log_norm, double *ess, double *mean, double *std,
                           double *quant, int *imaxL);
/* numpy.random.choice(F, n, p=p) of musefuse_postprocess.py:121 with numpy's own generator per data
 * set: index int32[ndata][n] equals Generator(Philox(key=[seed, first_column + d])).choice(F, size=n,
 * p=p) -- first_column: where the handle's columns start in the whole run (a .cols part of a sharded
 * run draws what the whole file would); xdraws double[ndata][n][ndim] (may be NULL) the drawn
 * x[index, d, :]. */
int mdns_posterior_resample(mdns_posterior *h, unsigned long long seed, long long first_column,
                            int n, int *index, double *xdraws);
/* device milliseconds of the last calls, from events: [0] max and weighted sums, [1] std,
 * [2] quantiles, [3] resampling (ms double[4]) */
int mdns_posterior_timings(const mdns_posterior *h, double *ms);

/* ------------------------------------------------------------------------------------------
 * Part 8 -- a polynomial continuum per spectrum in the scale-marginalised likelihood
 * (csrc/mdns_continuum.hip).
 *
 * With w = 1/v, basis b_k(x_j) = Legendre P_k(t_j), k < P, t_j = (2 x_j - x_0 - x_last) / (x_last - x_0):
 *   once per spectrum:        G = sum_j w b b^T, beta = G^-1 sum_j w b y, yt = y - sum_k beta_k b_k;
 *   per (template m, spectrum): alpha = G^-1 sum_j w b m, mt = m - sum_k alpha_k b_k,
 *                             s = sum w yt mt / (1e-10 + sum w mt^2), L = -0.5 sum w (yt - s mt)^2;
 * the least-squares minimum over (s, c_0..c_{P-1}) of sum w (y - s m - sum c_k b_k)^2, fitted continuum
 * c = beta - s alpha.  The bits of L for a (template, spectrum) pair do not depend on B, M, the pair's place in
 * its batch or the entry point.
 *
 * mdns_spectra_set_continuum: P = 0 switches the continuum off, 1..4 on; the spectra need variances and a
 * wavelength grid.  While P > 0 EVERY scale-marginalised scoring on the handle -- mdns_muse_loglike_batch[_dev],
 * mdns_muse3_/mdns_lines_loglike_batch[_dev], the joint state and its draw chunks in both forms -- is this
 * likelihood; chunks take the dense route (no matrix-core filter: mdns_muse_filter_dev fails).  Refused once a
 * joint state exists on the handle.  A spectrum with fewer than P channels that carry weight (or nx < P) fails
 * the call with a message naming the first such spectrum; the former setting stays in force.
 * mdns_spectra_continuum: the current P (-1: null handle).
 *
 * mdns_muse_continuum_fit_batch[_dev]: templates ypred [B][nx] against the selected spectra as
 * mdns_muse_loglike_batch[_dev] scores them (the same kernel, the same bytes in Lout [B][M]), and the fit:
 * scale_out [B][M] = s, coef_out [B][M][P] = c.  The host form's three output pointers may each be NULL, of the
 * device form scale and coef.  0 on success, message in mdns_last_error().
 * ------------------------------------------------------------------------------------------ */
int mdns_spectra_set_continuum(mdns_spectra *s, int P);
int mdns_spectra_continuum(const mdns_spectra *s);
int mdns_muse_continuum_fit_batch(mdns_spectra *s, const double *ypred, int B, const int *row_ids, int M,
                                  double *Lout, double *scale_out, double *coef_out);
int mdns_muse_continuum_fit_batch_dev(mdns_spectra *s, const double *d_ypred, int B, const int *d_row_ids, int M,
                                      double *d_Lout, double *d_scale_out, double *d_coef_out);

/* ------------------------------------------------------------------------------------------
 * Part 9 -- caller-defined models at FIXED scale with per-pixel variances (csrc/mdns_curves.hip,
 * k_curve_rows_w).
 *
 *   L[b][k] = -0.5 * sum_j w[row_k][j] * (curves[b][j] - y[row_k][j])**2,   w = 1/v as the handle keeps it
 *
 * (the constant -0.5 sum log 2 pi v is omitted, as everywhere).  A pixel is masked by w = 0 -- v = inf -- with a
 * finite y: it then contributes nothing, bit for bit.  The amplitude of the model is the caller's parameter:
 * nothing is fitted per spectrum.  Per pair ONE chain over the channels in ascending order, from acc = +0:
 * d = c - y, t = w * d (rounded), acc = fma(t, d, acc); L = -0.5 * acc.  The bits of a pair do not depend on B, M,
 * its place in the batch, ldc or the entry point.  Curve values are not validated: non-finite ones propagate as IEEE.
 *
 * mdns_curve_chi2_batch[_dev]: arguments, size checks and messages as mdns_curve_loglike_batch[_dev] without the
 * noise level; pure functions of a handle WITH variances (else "spectra were created without variances"), in
 * whatever mode it is.  B == 0 or M == 0: nothing happens.
 *
 * mdns_spectra_set_fixed_scale(s, 1): every curve scoring of a joint state on this handle -- mdns_joint_init_curves,
 * mdns_backend_draw_curves[_dev] -- is this likelihood instead of the scale-marginalised one; jitter, accept, commit
 * and mailbox are the same.  Such a state takes curve chunks ONLY: mdns_joint_init_muse3, mdns_backend_draw_chunk,
 * mdns_backend_draw_score and mdns_backend_draw_band[_begin] fail on it (and leave it usable).  The pure batch
 * functions (mdns_muse_loglike_batch* ...) compute what their names say in either mode.  The setter fails -- the
 * former setting stays in force -- on a handle without variances, once a joint state exists on the handle, and
 * while a continuum is set; mdns_spectra_set_continuum(P > 0) fails on a fixed-scale handle.
 * mdns_spectra_fixed_scale: the current setting (-1: null handle).
 * ------------------------------------------------------------------------------------------ */
int mdns_curve_chi2_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout);
int mdns_curve_chi2_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                              double *d_Lout);
int mdns_spectra_set_fixed_scale(mdns_spectra *s, int on);
int mdns_spectra_fixed_scale(const mdns_spectra *s);

/* ------------------------------------------------------------------------------------------
 * Part 10 -- caller-defined models against PHOTON COUNTS: the Poisson likelihood, the "C statistic" of X-ray
 * fitting (csrc/mdns_curves.hip, k_curve_log + k_curve_rows_p).
 *
 * Per spectrum k and channel j: counts n >= 0 (the handle's y; finite, not necessarily integers) and an exposure
 * e >= 0 (effective area x time, flat field ...; e = 0 masks the pixel).  A curve c >= 0 is the expected count RATE
 * per unit exposure, the expected counts are e c.  With tiny = DBL_MIN:
 *
 *   L[b][k] = sum_j ( n[row_k][j] * log(max(curves[b][j], tiny)) - e[row_k][j] * curves[b][j] ) + K[row_k]
 *   K[k]    = sum over the pixels with n > 0 and e > 0 of  n (1 + log e - log n)        (the caller's, see below)
 *
 * For c > 0 that is -C/2 with C = 2 sum (e c - n + n log(n / (e c))): <= 0, and 0 for a perfect model (log n! is
 * omitted, as every constant is).  Per pair ONE chain over the channels in ascending order, from acc = +0:
 * acc = fma(n, lc, acc), acc = fma(-e, c', acc); L = acc + K, where k_curve_log made lc = log(max(c', tiny)) and
 * c' = c once per candidate and channel.  The bits of a pair do not depend on B, M, its place in the batch, ldc or
 * the entry point.
 *   zero model     c = +-0 where n = 0 contributes exactly nothing; where n > 0 it costs n log(tiny), about -708 n:
 *                  finite and ordered.
 *   invalid model  a negative or NaN curve value (c' = NaN) makes L NaN for EVERY spectrum, masked pixel or not;
 *                  the accept test of a joint state rejects NaN.  +inf is not validated.
 *   masked pixel   n = 0 and e = 0: a deleted channel, bit for bit, for every finite c >= 0.  A spectrum without a
 *                  good pixel scores K = 0, hence +0.0.
 *
 * mdns_spectra_set_counts(s, exposure, offsets): puts a handle created WITHOUT variances into counts mode.
 * exposure f64[ndata][nx] (one spectrum per row, contiguous), or NULL for all ones; offsets f64[ndata], the K[k] --
 * computed by the caller, so that no device logarithm enters them --, or NULL for zeros.  Both go into buffers of
 * their own on the handle, and y is zeroed where e == 0 (with what the handle keeps derived from y).  Fails -- the
 * handle stays as it was -- on a null handle, on a handle created with variances, once a joint state exists on the
 * handle, and when an exposure is negative or not finite (looked for in the host array before anything is
 * uploaded).  There is no way back out of the mode.  mdns_spectra_counts: 0 or 1 (-1: null handle).
 *
 * mdns_curve_poisson_batch[_dev]: arguments, size checks and messages as mdns_curve_chi2_batch[_dev]; on a handle
 * that is not in counts mode "spectra are not in counts mode (mdns_spectra_set_counts)".  B == 0 or M == 0: nothing
 * happens.
 *
 * A joint state created on a counts handle takes the dense route of the scale-marginalised likelihood; every curve
 * scoring of it -- mdns_joint_init_curves, mdns_backend_draw_curves[_dev] -- is this likelihood; jitter, accept,
 * commit and mailbox are the same.  Such a state takes curve chunks ONLY: mdns_joint_init_gauss,
 * mdns_joint_init_muse3, mdns_backend_draw_chunk, mdns_backend_draw_score, mdns_backend_draw_band[_begin] and
 * mdns_joint_score_dev fail on it with "counts spectra take curve chunks only ..." (and leave it usable).
 * mdns_spectra_set_fixed_scale and mdns_spectra_set_continuum(P > 0) fail on the handle as on any without
 * variances.  The Gaussian batch functions (mdns_gauss_loglike_batch, mdns_curve_loglike_batch*) keep computing what
 * their names say, from the y that is on the handle.
 * ------------------------------------------------------------------------------------------ */
int mdns_spectra_set_counts(mdns_spectra *s, const double *exposure, const double *offsets);
int mdns_spectra_counts(const mdns_spectra *s);
int mdns_curve_poisson_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout);
int mdns_curve_poisson_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                 double *d_Lout);

/* ------------------------------------------------------------------------------------------
 * Part 11 -- caller-defined models against photon counts WITH A BACKGROUND SPECTRUM: the W statistic of X-ray
 * fitting (csrc/mdns_curves.hip, k_curve_rows_b).
 *
 * Per spectrum k and channel j, beside the source region's counts n and exposures e of Part 10 (which hold source plus
 * background): the background region's counts b >= 0 and its exposure g >= 0, the area ratio included, so that g f is
 * the expected background count in the background region for a background rate f.  f is unknown, one per pixel, and
 * profiled out of the joint Poisson likelihood of the two spectra in closed form.  The curve c >= 0 is the SOURCE count
 * rate per unit exposure; c' = c for c >= 0 (-0 included) and NaN otherwise; tiny = DBL_MIN.  Per pixel
 *
 *   T = e + g;  N = n + b;  Q = 4 (T b);  T2 = 2 T (1 where T == 0);  b2 = 2 b           (each one rounded operation)
 *
 * and per (candidate, spectrum, channel), every operation a rounded fp64 one in this order:
 *
 *   a = fma(-T, c', N);  d = sqrt(fma(a, a, Q c'))
 *   f = (a + d) / T2   where a >= 0
 *   f = (b2 c') / (d - a)   where not           (the naive form loses every digit for T c' >> N)
 *   s = c' + f
 *   acc = fma(n, log(max(s, tiny)), acc);  acc = fma(b, log(max(f, tiny)), acc);  acc = fma(-e, s, acc);  acc = fma(-g, f, acc)
 *
 *   L[b][k] = acc over the channels in ascending order from acc = +0, + Kw[row_k]
 *   Kw[k]   = sum over n > 0 of n (1 + log e - log n)  +  sum over b > 0 of b (1 + log g - log b)      (the caller's)
 *
 * That is -W/2: <= 0, and 0 where model plus fitted background reproduce both spectra.  In exact arithmetic f = b/T for
 * n = 0, f = max(n/T - c', 0) for b = 0, f = 0 for n = b = 0; where b = 0 and c' >= n/T the term is Part 10's.  The
 * bits of a pair do not depend on B, M, its place in the batch, ldc, the grid split or the entry point; log, sqrt and /
 * are the device library's fp64 ones.
 *   masked pixel   n = e = b = g = 0: T2 = 1, f = 0 / 1 = 0, a deleted channel, bit for bit, for every finite c >= 0.
 *                  A spectrum without a good pixel scores Kw = 0, hence +0.0.
 *   zero model     c = +-0 where n > 0, b = 0 gives f = n/T > 0: finite, no penalty.  Where n = b = 0 it contributes
 *                  exactly nothing.
 *   invalid model  a negative or NaN curve value makes L NaN for EVERY spectrum, masked pixels or not, and for no
 *                  other candidate of the batch.  +inf is not validated.
 *
 * mdns_spectra_set_background(s, bkg_counts, bkg_exposure, offsets): gives a handle that is in counts mode its
 * background.  bkg_counts f64[ndata][nx] (one spectrum per row, contiguous); bkg_exposure the same shape, or NULL for
 * all ones; offsets f64[ndata], the Kw[k] -- the caller's, so that no device logarithm enters them --, or NULL for
 * zeros.  A pixel whose g is 0 or NaN, or whose b is not finite, or which is masked on the handle already (e = 0), is
 * masked on both sides: n, e, b and g become 0, with what the handle keeps derived from y.  Fails -- the handle stays as
 * it was -- on a null handle, on a handle that is not in counts mode, once a joint state exists on the handle, on null
 * counts, and when an exposure is negative or infinite or a count of an unmasked pixel negative (looked for in the host
 * arrays before anything is uploaded; the message names the index).  There is no way back, and mdns_spectra_set_counts
 * fails on a handle that has a background.  mdns_spectra_background: 0 or 1 (-1: null handle).
 *
 * mdns_curve_wstat_batch[_dev]: arguments, size checks and messages as mdns_curve_poisson_batch[_dev]; on a handle
 * without a background "spectra have no background (mdns_spectra_set_background)".  B == 0 or M == 0: nothing happens.
 * mdns_curve_background_batch[_dev]: the same arguments, fout f64[B][M][nx] = the f of every pixel, made by the device
 * functions the scoring kernel uses (0 at a masked pixel; NaN along an invalid curve value).
 *
 * A joint state on such a handle is Part 10's with this likelihood for every curve scoring; it takes curve chunks
 * only.  mdns_curve_poisson_batch[_dev] on such a handle keep computing what their name says: the C statistic of the n,
 * e and K that are on it.
 * ------------------------------------------------------------------------------------------ */
int mdns_spectra_set_background(mdns_spectra *s, const double *bkg_counts, const double *bkg_exposure, const double *offsets);
int mdns_spectra_background(const mdns_spectra *s);
int mdns_curve_wstat_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *Lout);
int mdns_curve_wstat_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                               double *d_Lout);
int mdns_curve_background_batch(mdns_spectra *s, const double *curves, int B, const int *row_ids, int M, double *fout);
int mdns_curve_background_batch_dev(mdns_spectra *s, const double *d_curves, int ldc, int B, const int *d_row_ids, int M,
                                    double *d_fout);

/* ------------------------------------------------------------------------------------------
 * Part 12 -- a MODEL on the device: a tabulated template grid (csrc/mdns_table.hip, k_table_curves, k_table_los_*).
 *
 * The model of the reference's real workload (musefuse.py:222-284) and of X-ray table models: templates tabulated over
 * a few parameters, interpolated multilinearly, resampled at x / (1 + z) with numpy.interp's end rules, times an
 * amplitude.  The caller hands the table over once; the curves of a chunk are made on the device from the candidates'
 * parameters and never leave it on their way to the curve scoring of Parts 2, 9, 10 and 11.
 *
 * All float64.  axes: d arrays (1 <= d <= MDNS_TABLE_MAX_AXES), axis a of n_a >= 2 knots, finite, strictly increasing,
 * one after the other; grid f64[nw], nw >= 2, finite, strictly increasing: the templates' own abscissa; table
 * f64[n_1] .. [n_d][nw], C order, finite, any sign; x f64[nx], finite: the abscissa of the data.  A candidate is the
 * row (p_1 .. p_d [, z] [, A]): z with MDNS_TABLE_REDSHIFT, A with MDNS_TABLE_AMPLITUDE, ndim = d + the flags set.
 *
 * Per candidate, every step ONE rounded fp64 operation, in this order, nothing contracted into an FMA:
 *
 *   cell      v_a = p_a clamped to [axis_a[0], axis_a[n_a - 1]]   (v < lo ? lo : v > hi ? hi : v: +-inf clamp)
 *             i_a = the last knot <= v_a, at most n_a - 2;   f_a = (v_a - axis_a[i_a]) / (axis_a[i_a + 1] - axis_a[i_a])
 *   weights   for corner c = 0 .. 2^d - 1 (bit a of c set: knot i_a + 1):  w_c = 1, then for a ascending
 *             w_c = w_c * (bit a set ? f_a : 1 - f_a)
 *   abscissa  u_j = x_j / (1 + z) (without the flag u_j = x_j), clamped to [grid[0], grid[nw - 1]] in the same way;
 *             k_j = the last knot <= u_j, at most nw - 2;   t_j = (u_j - grid[k_j]) / (grid[k_j + 1] - grid[k_j])
 *   value     acc = 0, then for c ascending  acc = acc + w_c * (T_c[k_j] + t_j * (T_c[k_j + 1] - T_c[k_j]))
 *             with T_c the table row of corner c;   curve[b][j] = A * acc (without the flag acc)
 *
 * A NaN in ANY parameter of a candidate makes its whole row NaN (and no other row): under every curve statistic such
 * a candidate is never accepted.  z = -1 gives u = +-inf, which clamps (where x_j = 0 as well, u_j = 0 / 0 and that
 * channel is NaN).  A value does not depend on B, on the candidate's place in the batch, on ldc or on the entry point;
 * / is the device's correctly rounded fp64 division.  The numpy statement of the same chain is
 * massivedatans_amd/tablemodel.py, TableModel.statement: the two agree bit for bit.
 *
 * mdns_table_create: copies everything to the device; the handle owns its blocks.  All or none: NULL (mdns_last_error
 * says why) and nothing left allocated when an argument is null, a size is outside its cap below, a knot, x or table
 * value is not finite, an axis or the grid is not strictly increasing (the message names the array and the index),
 * flags holds an unknown bit, or the device refuses.  Every rule is looked for in the host arrays before the device is
 * asked for anything.  mdns_table_nparams: ndim; mdns_table_nx: nx (-1: null handle).
 *
 * mdns_table_curves_batch: params host f64[B][ndim] -> out host f64[B][nx] (synchronous).  _dev: device pointers,
 * rows of ldc >= nx doubles whose padding is not touched, asynchronous on the library stream.  B == 0: nothing happens.
 *
 * mdns_backend_draw_table: mdns_backend_draw_curves (Part 5) with the curves of params host f64[B][ndim] made by the
 * table on the library's stream into a buffer of the joint state's: the same checks, then exactly the path of
 * mdns_backend_draw_curves_dev -- whichever curve statistic the state's spectra select.  Refuses a null table and one
 * whose nx is not the spectra's.  mdns_joint_init_table: mdns_joint_init_curves with the live points' curves made from
 * params f64[nlive][ndim] in the same way.
 *
 * LINE-OF-SIGHT EFFECTS (mdns_table_create_los).  The reference's model has two more parameters of this kind
 * (musefuse.py:222-284): an attenuation 10 ** (c(lambda) * EBV) of the rest-frame template, and a Gaussian velocity
 * broadening of it before the resampling.  MDNS_TABLE_EXTINCTION adds the parameter E, MDNS_TABLE_BROADEN the parameter
 * s (the velocity dispersion sigma_v / c, dimensionless); the candidate's row is (p_1 .. p_d [, z] [, E] [, s] [, A]),
 * ndim = d + the flags set.  ext f64[nw], finite, required with MDNS_TABLE_EXTINCTION: the exponent per unit E at each
 * template knot (the caller passes e.g. -0.4 k(lambda)).  MDNS_TABLE_BROADEN requires grid[0] > 0.  10 ** v below is
 * pow10_dd of csrc/mdns_pow10.h, one faithful rounding that host and device compute identically, so this stays a chain
 * of single rounded fp64 operations (the fma() calls inside pow10_dd are part of that function's definition).
 *
 * With neither new flag nothing changes: the statement above, its kernel and its bits.  With either, cell, f_a, w_c,
 * u_j, k_j, t_j and the clamps are as above and the value is blend, attenuate, broaden, interpolate:
 *
 *   blend     for a template knot m:  S_m = 0, then for c ascending  S_m = S_m + w_c * T_c[m]
 *   attenuate (MDNS_TABLE_EXTINCTION)  q = ext[m] * E, clamped to [-299, 299] by the same comparisons;
 *             S_m = S_m * pow10_dd(q)
 *   broaden   (MDNS_TABLE_BROADEN)  widths, made once at creation:  D_n = (grid[n + 1] - grid[n - 1]) * 0.5 inside,
 *             D_0 = (grid[1] - grid[0]) * 0.5,  D_{nw-1} = (grid[nw - 1] - grid[nw - 2]) * 0.5.
 *             s == 0:  R_m = S_m exactly.   s > 0:  d_mn = ((grid[n] - grid[m]) / grid[m]) / s;  the window of m is the
 *             contiguous run of n around m with |d_mn| <= MDNS_TABLE_BROADEN_CUT (d_mn is monotone in n and d_mm = 0);
 *             K_n = pow10_dd((MDNS_TABLE_BROADEN_C * d_mn) * d_mn) * D_n;  num = 0, den = 0, then for n ascending over
 *             the window  num = num + S_n * K_n,  den = den + K_n;  R_m = num / den.  A window cut by an end of the
 *             grid normalises over what is there.  Without the flag R = S.
 *   value     curve[b][j] = R_{k_j} + t_j * (R_{k_j + 1} - R_{k_j}), times A with MDNS_TABLE_AMPLITUDE (A * value)
 *
 * The divisions of d_mn are divisions (no reciprocal).  The window has NO cap: a large s on a dense grid costs O(nw)
 * per template knot and O(nw^2) per candidate.  A NaN in any parameter makes the whole row NaN, as above; so does an E
 * that is not finite, and an s that is not finite or negative; no other row is touched.  A value depends on its
 * candidate and channel only -- not on B, the candidate's place in the batch, ldc, the entry point, or what the handle
 * computed before.  Extinction alone is one gather kernel of k_table_curves' shape (k_table_los_gather: a channel needs
 * S at its two knots only); with broadening three kernels follow each other on the library stream (k_table_los_blend
 * S[B][nw], k_table_los_broaden R[B][nw], k_table_los_resample), S and R grow-only blocks of the handle: a growth the
 * device refuses fails that call and leaves the handle usable.
 *
 * mdns_table_create_los: mdns_table_create with the two flags and ext (NULL without MDNS_TABLE_EXTINCTION); the same
 * rules, all or none, looked for in the host arrays first, and beside them: ext null with the flag, ext[i] not finite,
 * grid[0] <= 0 with MDNS_TABLE_BROADEN.  mdns_table_create takes neither new flag (flags=4: unknown bits).  Every other
 * entry of this part takes the handles of both.
 *
 * Not covered: more than MDNS_TABLE_MAX_AXES axes, interpolation other than linear, a broadening kernel other than a
 * Gaussian, extinction laws with more than one parameter, sharded runs, the chained first batch.
 * ------------------------------------------------------------------------------------------ */
#define MDNS_TABLE_MAX_AXES 4
#define MDNS_TABLE_MAX_NX (1 << 20)            /* channels of x at most                                  */
#define MDNS_TABLE_MAX_ELEMS 2147483647LL      /* table values at most (and knots of all axes together)   */
#define MDNS_TABLE_TILE 256                    /* channels (template knots) per workgroup of the kernels  */
#define MDNS_TABLE_REDSHIFT 1
#define MDNS_TABLE_AMPLITUDE 2
#define MDNS_TABLE_EXTINCTION 4
#define MDNS_TABLE_BROADEN 8
#define MDNS_TABLE_BROADEN_CUT 5.0             /* the Gaussian's window: |d_mn| <= this many sigmas       */
#define MDNS_TABLE_BROADEN_C (-0x1.bcb7b1526e50ep-3) /* the double nearest to -0.5 log10(e)                */
typedef struct mdns_table mdns_table;
mdns_table *mdns_table_create(const double *x, int nx, int d, const int *n, const double *axes, int nw, const double *grid,
                              const double *table, int flags);
mdns_table *mdns_table_create_los(const double *x, int nx, int d, const int *n, const double *axes, int nw, const double *grid,
                                  const double *table, int flags, const double *ext);
void mdns_table_destroy(mdns_table *t);
int mdns_table_nparams(const mdns_table *t);
int mdns_table_nx(const mdns_table *t);
int mdns_table_curves_batch(mdns_table *t, const double *params, int B, double *out);
int mdns_table_curves_batch_dev(mdns_table *t, const double *d_params, int B, double *d_out, int ldc);
int mdns_backend_draw_table(void *joint, mdns_table *table, const double *params, int B, const double *jitter, int *accepted,
                            unsigned long long *fillbits, int *nscored);
int mdns_joint_init_table(mdns_joint *j, mdns_table *table, const double *params, double noise_level, const double *jitter);

/* ------------------------------------------------------------------------------------------
 * Part 13 -- the INSTRUMENT RESPONSE on the device: model curves folded onto the data's channels before any statistic
 * sees them (csrc/mdns_response.hip, k_response_fold).
 *
 * Count spectra of real instruments are not measured on the model's bins: the model lives on n_in fine energy (or
 * wavelength) bins, the data on nx detector channels, and between the two sits a sparse, mostly banded matrix -- RMF x
 * ARF in X-ray fitting, a wavelength-dependent line-spread function for a spectrograph.  A response handle holds that
 * matrix; attached to a spectra handle, every curve entry of Parts 2, 5, 8, 9, 10, 11 and 12 takes curves of n_in bins
 * and folds them first, on the library stream, between "make curves" and "score curves".  A spectra handle without a
 * response behaves exactly as before.
 *
 * The matrix, CSR by channel:  rowptr i64[nx + 1], rowptr[0] = 0, non-decreasing, rowptr[nx] = nnz;  cols i32[nnz],
 * strictly increasing inside a row, in [0, n_in);  vals f64[nnz], finite, any sign.
 *
 *   folded[b][j] = acc,  where acc = +0.0, then for p = rowptr[j] .. rowptr[j + 1] - 1 ascending
 *                  acc = acc + vals[p] * curve[b][cols[p]]
 *
 * Each multiply and each add is ONE rounded fp64 operation, never contracted into an FMA.  An empty row gives +0.0.  A
 * NaN or inf in a bin is seen by exactly the channels whose rows hold that bin.  A value depends on its candidate and
 * channel only -- not on B, the candidate's place in the batch, ldc, the entry point, or what the handle computed
 * before.  The matrix cores are not used: their accumulation order is not this one.  The numpy statement of the same
 * chain is massivedatans_amd/response.py, Response.statement: the two agree bit for bit.
 *
 * mdns_response_create: every rule above is looked for in the host arrays before the device is asked for anything, and
 * the message names the array and the index; 1 <= nx, n_in <= MDNS_TABLE_MAX_NX, nnz <= 2^31 - 1.  The matrix is
 * re-laid per group of 64 channels so that entry l of the 64 rows is contiguous (one length per row; padding is never
 * multiplied) and copied to the device.  All or none: NULL (mdns_last_error says why) and nothing left allocated.
 * mdns_response_nx, mdns_response_nin: the two sizes (-1: null handle).
 *
 * mdns_response_fold_batch: curves host f64[B][n_in] -> out host f64[B][nx], synchronous, through grow-only scratch of
 * the handle.  _dev: device pointers, rows of ldc >= n_in and ldo >= nx doubles whose padding is neither read nor
 * written, asynchronous on the library stream.  B == 0: nothing happens.
 *
 * mdns_spectra_set_response(s, r): from now on every entry that takes model curves for s takes n_in bins per curve
 * (ldc >= n_in; the host forms rows of exactly n_in) and folds them into a grow-only buffer of s before it scores:
 * mdns_curve_loglike_batch, mdns_curve_chi2_batch, mdns_curve_poisson_batch, mdns_curve_wstat_batch and their _dev
 * forms, mdns_curve_background_batch[_dev], mdns_muse_loglike_batch[_dev] and mdns_muse_continuum_fit_batch[_dev] (the
 * scale-marginalised likelihood of curves, without and with a continuum), mdns_joint_init_curves,
 * mdns_backend_draw_curves[_dev], mdns_joint_init_table and mdns_backend_draw_table -- the last two then require the
 * table's nx to equal n_in.  No scoring kernel changes.  r == NULL detaches.  Refused: a response whose nx is not the
 * spectra's, and any change while a joint state lives on s.  The spectra handle BORROWS the response, which counts its
 * attachments: mdns_response_destroy of an attached response is refused (returns 1, frees nothing); detaching or
 * destroying the spectra releases it.  A growth of the folded buffer that the device refuses fails that call and leaves
 * the handles usable.
 *
 * Not covered: a response per spectrum (per-spectrum effective area goes into the exposures of Part 10), sharded runs,
 * the chained first batch.
 * ------------------------------------------------------------------------------------------ */
typedef struct mdns_response mdns_response;
mdns_response *mdns_response_create(int nx, int n_in, const long long *rowptr, const int *cols, const double *vals);
int mdns_response_destroy(mdns_response *r);
int mdns_response_nx(const mdns_response *r);
int mdns_response_nin(const mdns_response *r);
int mdns_response_fold_batch(mdns_response *r, const double *curves, int B, double *out);
int mdns_response_fold_batch_dev(mdns_response *r, const double *d_curves, int ldc, int B, double *d_out, int ldo);
int mdns_spectra_set_response(mdns_spectra *s, mdns_response *r);

/* ------------------------------------------------------------------------------------------
 * Part 14 -- a SUM of components as the model, evaluated on the device (csrc/mdns_sum.hip, k_sum_curves).
 *
 * Real analyses fit sums: absorption x (power law + line) + scattered table, population A + population B + emission
 * line.  A sum model has 1 <= C <= MDNS_SUM_MAX_COMPONENTS components in the order they were added -- a table of Part
 * 12 (MDNS_SUM_TABLE), a power law (MDNS_SUM_POWERLAW), a Gaussian line (MDNS_SUM_GAUSS) --, each with a flag
 * `attenuated`, and optionally ONE common attenuation factor.  It lives on an abscissa x f64[nx], finite, 1 <= nx <=
 * MDNS_TABLE_MAX_NX: the data's x, or under a response (Part 13) its model bins.  All float64.
 *
 * A candidate's row is the components' parameters one after the other in that order and, with an attenuation, N at the
 * end; ndim = the components' parameters + (attenuation ? 1 : 0) <= MDNS_MAX_DIM.
 *
 * Per candidate b and bin j, every step ONE rounded fp64 operation, in this order, nothing contracted into an FMA
 * (10 ** v is pow10_dd of csrc/mdns_pow10.h, one faithful rounding that host and device compute identically; the fma()
 * calls inside it belong to that function); clamp is Part 12's comparison clamp to [-299, 299]:
 *
 *   TABLE     parameters: Part 12's row (p_1 .. p_d [, z] [, E] [, s] [, A]).  v = exactly Part 12's value for that
 *             slice of the row on x, by either of its routes.
 *   POWERLAW  parameters (logA, G); lx f64[nx], finite, given at creation (the Python layer: log10(x / x0)).
 *             q = G * lx[j];  q = logA - q;  q = clamp(q);  v = pow10_dd(q)
 *   GAUSS     parameters (A, mu, sigma): the peak amplitude, as the reference's line (sample.py:60-62).
 *             d = (x[j] - mu) / sigma;  q = (MDNS_TABLE_BROADEN_C * d) * d;  q = clamp(q);  v = A * pow10_dd(q)
 *             It is not cut: far from the line the value is A * 1e-299, not 0.
 *   sums      a = +0.0, then for the attenuated components ascending  a = a + v_c;
 *             u = +0.0, then for the others ascending  u = u + v_c.
 *             Without an attenuation every component counts as attenuated.
 *   attenuate (optional; att f64[nx], finite)  q = clamp(att[j] * N);  a = a * pow10_dd(q)
 *   value     curve[b][j] = a + u
 *
 * A NaN anywhere in the row makes the whole row NaN.  So does a parameter of an analytic component that is not finite,
 * a sigma that is not > 0, and an N that is not finite.  A table slice follows Part 12's own rules: a slice that Part 12
 * makes NaN is NaN in every bin and so is the sum.  A NaN's payload is not part of the statement.  With finite
 * parameters no step of a component's chain or of the attenuation can produce a NaN: G * lx, x - mu and att * N may
 * overflow to +-inf, logA - q and d then stay infinite (sigma is finite and > 0, so d is never inf / inf; d = 0 gives
 * q = -0.0 and pow10_dd(+-0.0) = 1), and the clamp catches them; pow10_dd of a clamped q lies in [1e-299, 1e299], so
 * A * pow10_dd(q) is finite and a * pow10_dd(q) is 0 * finite or +-inf * positive at worst.  The ADDS alone can: partial
 * sums beyond 1.8e308 of opposite sign in a and u give inf + -inf.  A value depends on its candidate and bin only --
 * not on B, the candidate's place in the batch, ldc, the entry point, or what the handle computed before.  A model of
 * one TABLE component without attenuation gives the table's own curves, except that -0.0 becomes +0.0 (0.0 + -0.0).
 * The numpy statement of the same chain is massivedatans_amd/summodel.py, SumModel.statement: the two agree bit for bit.
 *
 * mdns_sum_create: copies x; NULL (mdns_last_error says why) for a null x, nx outside 1 .. MDNS_TABLE_MAX_NX, x[i] not
 * finite, or a device that refuses.  The sum OWNS what its components need: mdns_sum_add_table takes
 * mdns_table_create_los's arguments and builds that table on the sum's own x (every rule and message of Part 12, under
 * the name mdns_sum_add_table); mdns_sum_add_powerlaw copies lx; mdns_sum_add_gauss needs nothing;
 * mdns_sum_set_attenuation copies att.  Adding is all or none: a refused call (returns 1) leaves the model as it was and
 * nothing allocated; every rule is looked for in the host arrays before the device is asked for anything, and the
 * message names the function, the array and the index.  Refused: a null argument; lx[i] or att[i] not finite; a ninth
 * component; ndim above MDNS_MAX_DIM; a second mdns_sum_set_attenuation; any add or set_attenuation after the handle's
 * first use -- a curves, init or draw call that got as far as making curves -- ("the model is fixed at its first use");
 * a model without components in any curves, init or draw call.  mdns_sum_destroy frees the tables with the rest.
 * mdns_sum_nparams: ndim; mdns_sum_nx; mdns_sum_ncomponents (-1: null handle).
 *
 * mdns_sum_curves_batch: params host f64[B][ndim] -> out host f64[B][nx] (synchronous).  _dev: device pointers, rows of
 * ldc >= nx doubles whose padding is not touched, asynchronous on the library stream.  B == 0: nothing happens.  The
 * table components' curves go through a grow-only block [tables][B][nx] of the handle: a growth the device refuses fails
 * that call and leaves the handle usable.  One launch_table_curves per table component (1 or 3 kernels each), then ONE
 * k_sum_curves, grid (B, ceil(nx / MDNS_TABLE_TILE)), a bin per thread.
 *
 * mdns_backend_draw_sum, mdns_joint_init_sum: mdns_backend_draw_table and mdns_joint_init_table with the curves made by
 * the sum: the same checks, then exactly the path of mdns_backend_draw_curves_dev, under every curve statistic, with or
 * without a response.  Refused beside the above: a sum whose nx is not the spectra's, or not the response's n_in where
 * one is attached.  No scoring, accept or commit kernel changes.
 *
 * Not covered: parameters shared between components (one redshift for a table and a line), bin-integrated components,
 * components other than these three, more than one attenuation, sharded runs, the chained first batch.
 * ------------------------------------------------------------------------------------------ */
#define MDNS_SUM_MAX_COMPONENTS 8
#define MDNS_SUM_TABLE 0
#define MDNS_SUM_POWERLAW 1
#define MDNS_SUM_GAUSS 2
typedef struct mdns_sum mdns_sum;
mdns_sum *mdns_sum_create(const double *x, int nx);
int mdns_sum_add_table(mdns_sum *m, int d, const int *n, const double *axes, int nw, const double *grid, const double *table,
                       int flags, const double *ext, int attenuated);
int mdns_sum_add_powerlaw(mdns_sum *m, const double *lx, int attenuated);
int mdns_sum_add_gauss(mdns_sum *m, int attenuated);
int mdns_sum_set_attenuation(mdns_sum *m, const double *att);
void mdns_sum_destroy(mdns_sum *m);
int mdns_sum_nparams(const mdns_sum *m);
int mdns_sum_nx(const mdns_sum *m);
int mdns_sum_ncomponents(const mdns_sum *m);
int mdns_sum_curves_batch(mdns_sum *m, const double *params, int B, double *out);
int mdns_sum_curves_batch_dev(mdns_sum *m, const double *d_params, int B, double *d_out, int ldc);
int mdns_backend_draw_sum(void *joint, mdns_sum *m, const double *params, int B, const double *jitter, int *accepted,
                          unsigned long long *fillbits, int *nscored);
int mdns_joint_init_sum(mdns_joint *j, mdns_sum *m, const double *params, double noise_level, const double *jitter);

#ifdef __cplusplus
}
#endif
#endif /* MDNS_H */
