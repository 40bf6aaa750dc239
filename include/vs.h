/*
 * vs.h -- C ABI of the MI355X-native exact flat k-NN backend (libvs.so).
 *
 * Drop-in boundary for the vector arithmetic behind the reference's VectorStore
 * (/root/reference/utils/vector_store.py).  The reference reaches faiss through SWIG at these
 * call sites; each entry point below replaces one of them:
 *
 *   faiss.IndexFlatIP(d) / faiss.IndexFlatL2(d)   utils/vector_store.py:79-81   -> vs_create
 *   index.add(vector)                             utils/vector_store.py:163-164 -> vs_add
 *   index.search(vector, k)                       utils/vector_store.py:190-191 -> vs_search
 *   index.reconstruct(i)                          utils/vector_store.py:207     -> vs_reconstruct
 *   index.ntotal / index.d                        utils/vector_store.py:183,188,255-258,271 -> vs_ntotal, vs_dim
 *   _create_index() on clear()                    utils/vector_store.py:277     -> vs_reset
 *   faiss.write_index (storage payload)           utils/vector_store.py:234     -> vs_reconstruct_n
 *
 * Plain pointers and sizes only; no torch types.  Rows are row-major n x d fp32, already
 * normalised by the Python layer exactly as the reference does it (utils/vector_store.py:83-90).
 *
 * Semantics of vs_search (faiss IndexFlat semantics, made exact):
 *   - IP: D descending, L2: D ascending (squared L2), ties -> lower id.
 *   - The returned ids are the exact top-k under the canonical fp64 score (oracle/vs_oracle.c);
 *     D is that score rounded to fp32 (|D - faiss fp32 D| <= 1e-5 for unit vectors).
 *   - Unfilled slots (k > ntotal): I = -1, D = -FLT_MAX (IP) / +FLT_MAX (L2).
 *
 * Errors: every int-returning function returns 0 on success, < 0 on failure; the message is
 * in vs_last_error() (thread-local).  No C++ exception crosses the ABI.
 *
 * Threading: concurrent vs_search* calls on one handle are safe (shared corpus, one stream +
 * workspace per call from a pool).  vs_add, vs_add_device, vs_add_synthetic, vs_reset and vs_remove_ids
 * take an exclusive lock.  vs_kmeans takes the shared lock for its whole run, as a search does: it may
 * run beside searches and other vs_kmeans calls on the handle (each call owns its streams, workspace
 * and temporary centroid index), while adds, resets and removals wait for it.
 */
#ifndef VS_H_
#define VS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vs_index vs_index;

enum { VS_METRIC_IP = 0, VS_METRIC_L2 = 1 };
enum { VS_DTYPE_F32 = 0, VS_DTYPE_BF16 = 1, VS_DTYPE_F16 = 2 };
enum { VS_SCREEN_NATIVE = 0, VS_SCREEN_I8 = 1 };

enum {
    VS_OK = 0,
    VS_ERR_ARG = -1,          /* bad argument (dims, k, null pointer) */
    VS_ERR_DEVICE = -2,       /* no HIP device / HIP runtime failure */
    VS_ERR_OOM = -3,          /* device allocation failed */
    VS_ERR_UNCERTIFIED = -4,  /* exactness certificate could not be established (IVF list search
                               * only: every flat search ends in the exact full scan instead) */
    VS_ERR_INTERNAL = -5
};

/* ---- lifecycle (faiss.IndexFlatIP / IndexFlatL2 constructors, utils/vector_store.py:79-81) */
int vs_create(int d, int metric, int dtype, int device, vs_index** out);
void vs_destroy(vs_index* index);
int vs_reset(vs_index* index);                    /* clear(): utils/vector_store.py:273-280 */

/* ---- add (index.add, utils/vector_store.py:164) */
int vs_add(vs_index* index, const float* x, int64_t n);                 /* host fp32 n x d */
int vs_add_device(vs_index* index, const float* x_dev, int64_t n, void* stream); /* device fp32, packed on
                                                                                  * `stream` (NULL: legacy default) */
/* Fill rows [ntotal, ntotal+n) with synthetic rows global_row0.. of the counter-hash generator
 * (bench / tests; bit-identical to oracle/vs_oracle.c orc_synth_rows). */
int vs_add_synthetic(vs_index* index, uint64_t seed, int64_t global_row0, int64_t n, int normalize);
/* Size the row storage (and the int8 screen copy) for n more rows in one allocation: later adds up
 * to that size never regrow (a regrow copies the rows into a 1.5x larger buffer, so the old and
 * the new storage coexist for the copy).  vs_capacity: rows the storage holds without regrowing. */
int vs_reserve(vs_index* index, int64_t n);
int64_t vs_capacity(const vs_index* index);
/* Same generator, written as row-major fp32 (values rounded to `dtype`) into device memory on
 * `device`: synthetic query batches for bench.py / tests. */
int vs_synthesize(int device, uint64_t seed, int64_t global_row0, int64_t n, int d, int normalize, int dtype,
                  float* out_dev, void* stream);

/* ---- search (index.search, utils/vector_store.py:191).  Exact for every query: a failed
 * certificate re-screens the query 4x deeper, and past the deepest screen (KP_MAX) the exact full
 * scan answers it (faiss's k lowest ids among any number of tied rows).  Value domain: exactness
 * holds, and is tested, for finite stored values with row and query norms zero or in [2^-40, 2^40];
 * beyond it (fp32 ||x||^2 under- or overflows, f16 rows saturate from 65520, scores leave fp32's
 * normal range) results are unspecified, and non-finite inputs are not validated. */
int vs_search(vs_index* index, const float* q, int64_t nq, int32_t k, float* D, int64_t* I);
/* All pointers device-resident; enqueued on `stream` (NULL = the legacy default stream, which is
 * torch's default stream: device calls are always ordered with the caller's stream), no host
 * sync.  S64 (optional, may be NULL) receives the exact fp64 scores; id_offset is added to every
 * returned id (row-sharded corpora).  Certification failures are counted on the device
 * (vs_uncertified_count) and are NOT retried on this path. */
int vs_search_device(vs_index* index, const float* q_dev, int64_t nq, int32_t k, float* D_dev,
                     int64_t* I_dev, double* S64_dev, int64_t id_offset, void* stream);

/* Same outputs, but exact for every query (every dtype): each query block's first pass is
 * followed on the stream by a fallback round at the deepest screen (KP_MAX, proven seed; the MFMA
 * screen of the stored dtype, fp32 included) whose kernels do nothing unless a certificate of that
 * block failed, and which rewrites only the failed queries; a query even that round cannot certify
 * (more near-tied rows than KP_MAX, e.g. thousands of identical embeddings) is answered by a gated
 * exact full scan of the shard (every row scored, a running top-k: faiss's lowest ids among any
 * number of ties; counted in vs_full_scan_count) -- no host sync: the call returns with the work
 * queued.  The product's multi-GPU layers (photo_search_engine_amd/distributed.py,
 * vs_multi_search) use this one. */
int vs_search_device_exact(vs_index* index, const float* q_dev, int64_t nq, int32_t k, float* D_dev,
                           int64_t* I_dev, double* S64_dev, int64_t id_offset, void* stream);

/* ---- two-phase exact device search: the sharded step (one shard per rank) with a global T'
 * exchange (no faiss counterpart; replaces vs_search_device_exact inside
 * photo_search_engine_amd/distributed.py when vs_two_phase_ok says so).
 *  phase A: screen the shard and score each query's best keys exactly; S_a / I_a (nq x k, device,
 *           best-first, ids + id_offset, padded with -1 / worst score) are this shard's best so far;
 *           returns a pending search in *out that holds the index's read lock and workspace;
 *  (the caller all-gathers every shard's (S_a, I_a) and merges them: vs_merge_shards_device)
 *  phase B: floor_S = that merged nq x k list (device): its k-th score per query is a lower bound
 *           of the global k-th best, so the shard scores only rows whose bound reaches it and
 *           certifies against it; writes the shard's exact top-k as vs_search_device_exact does
 *           (its gated device fallback round included) and frees the pending search.
 * Results after the final all-gather + merge are identical to vs_search_device_exact's.  Every rank
 * must take the same path: vs_two_phase_ok depends only on the index configuration (int8 screen,
 * bf16/f16 rows) and on (nq, k) -- one int8 MFMA block, 8 < nq <= 256, k <= 1024.  world = the
 * number of shards (sets phase A's depth).  stride: the element stride of the (S, I) outputs (2 =
 * interleaved (score bits, id) pairs, ready for the all-gather; D_dev stays nq x k).
 * vs_search_pending_free drops a pending search whose phase B will not run. */
typedef struct vs_pending vs_pending;
int vs_two_phase_ok(vs_index* index, int64_t nq, int32_t k);
int vs_search_device_phase_a(vs_index* index, const float* q_dev, int64_t nq, int32_t k, int32_t world,
                             int64_t id_offset, double* S_a, int64_t* I_a, int32_t stride, void* stream,
                             vs_pending** out);
int vs_search_device_phase_b(vs_pending* pending, const double* floor_S, float* D_dev, int64_t* I_dev,
                             double* S64_dev, int32_t stride, void* stream);
void vs_search_pending_free(vs_pending* pending);

/* ---- merge of per-shard results (all-gather + K3 merge).
 * S_in/I_in: G x nq x k (device), each list sorted best-first, element (g, q, j) at index
 * ((g * nq + q) * k + j) * in_stride (1 = separate arrays; 2 = one interleaved array of (score bits,
 * id) pairs, S_in = its base, I_in = base + 8 bytes: what one all-gather of packed pairs yields);
 * output nq x k best-first under (score desc | asc for L2, id asc).  D_out is S_out rounded to
 * fp32 (may be NULL). */
int vs_merge_shards_device(int metric, const double* S_in, const int64_t* I_in, int32_t in_stride, int G,
                           int64_t nq, int32_t k, double* S_out, int64_t* I_out, float* D_out, void* stream);

/* ---- the int8 / native MFMA screens' threshold seed, exposed for verification: for each of nq
 * queries, the rank-th largest of its M sampled maxima (device fp32 [nq][M]) as a starting key
 * (ordered fp32 << 32) in thr_dev[q] (device u64 [nq]); 0 when M < rank.  M <= 8192, rank >= 1. */
int vs_seed_select_device(int device, const float* maxima_dev, int32_t M, int64_t nq, int32_t rank,
                          uint64_t* thr_dev, void* stream);

/* ---- reconstruct (index.reconstruct, utils/vector_store.py:207) */
int vs_reconstruct(vs_index* index, int64_t id, float* out);
int vs_reconstruct_n(vs_index* index, int64_t i0, int64_t n, float* out); /* host n x d */

/* ---- persistence (faiss.read_index / faiss.write_index payloads, utils/vector_store.py:249, :234;
 * SURVEY.md §8 f3).  The host layer parses / writes the 45-byte IxFI/IxF2 header; these move the
 * row-major fp32 payload between the file and HBM through pinned double buffers (file reads and
 * writes overlap the PCIe copies and the pack / unpack kernels).
 * vs_add_from_file appends rows [0, n) of the payload at byte_offset (== index.add of them).
 * vs_write_rows_to_file writes stored rows [i0, i0+n) at byte_offset of `path` (created if absent,
 * never truncated): a full rewrite, or an append of the rows added since the last save. */
int vs_add_from_file(vs_index* index, const char* path, int64_t byte_offset, int64_t n);
int vs_write_rows_to_file(vs_index* index, const char* path, int64_t byte_offset, int64_t i0, int64_t n);

/* ---- screen selection (no reference counterpart: faiss IndexFlat has one exact scan).
 * VS_SCREEN_NATIVE (default): batches screen the stored rows (bf16/f16 MFMA, or the fp32 GEMV).
 * VS_SCREEN_I8: the index keeps an int8 copy of its rows (per-row scale, +1 byte per element,
 * built from the stored values now and on every add) and batches of > 8 queries with k <= 1024
 * screen it with int8 MFMAs under a proven per-row error bound; an adaptive exact refine then
 * scores every candidate the bound cannot exclude.  Results are identical to the native path
 * (same exact ids and scores); queries the certificate rejects are re-searched natively.
 * Both metrics: L2 keys bound the transformed score 2 <x, q> - ||x||^2 from above (the fp32 row
 * norm and its rounding inside the margin), and the refine compares canonical distances. */
int vs_set_screen(vs_index* index, int screen);
int vs_screen(const vs_index* index);

/* ---- introspection */
int64_t vs_ntotal(const vs_index* index);
int vs_dim(const vs_index* index);
int vs_metric(const vs_index* index);
int vs_dtype(const vs_index* index);
int vs_device(const vs_index* index);
const char* vs_last_error(void);
const char* vs_version(void);

/* ---- measurement hooks (bench.py): HIP events around the dominant screen kernel, recorded on
 * the stream it is launched on.  vs_timing_fetch synchronises those events and returns up to
 * `cap` per-launch durations (ms), oldest first, then clears them. */
int vs_set_timing(vs_index* index, int enable);
/* Calls of 1-2 queries with k <= 64 over an index of at most 65536 rows and at most `bytes` stored
 * bytes (rows x padded d x element size; default 192 MiB) skip the screen: one launch scores every
 * row exactly and selects the top-k (the full scan of vs_search_device_exact's last tier, run
 * first) -- the product's single-query call on a photo library, BASELINE cfg1.  0 = always screen
 * (tests of the screen kernels).  Results are the same bits either way. */
int vs_set_scan_limit(vs_index* index, int64_t bytes);
/* One launch of the main screen kernel (screen = VS_SCREEN_I8: the int8 direct screen; NATIVE: the
 * bf16 / f16 direct screen) over the whole index for 9..256 device queries, every query's threshold
 * at +inf (the bound test passes nothing: the K loop + epilogue test, no survivors); zero_queries
 * zeroes the packed query tile first, so one MFMA operand is all zeros.  Five launches back to
 * back; *ms = the fastest one's duration (HIP events on `stream`, synchronised).  bench.py runs both forms in the same process as the timed
 * steps: the box's own zero / real operand pair behind the power note of its roofline. */
int vs_screen_probe(vs_index* index, const float* q_dev, int64_t nq, int32_t screen, int32_t zero_queries,
                    void* stream, float* ms);
/* Diagnostic forms of the direct screen's loop (csrc/vs_k1probe.hip; DESIGN §5 "Where K1 int8's time
 * goes"), over the whole index like vs_screen_probe (thresholds at +inf, 9..256 device queries,
 * zero_queries as there).  screen = VS_SCREEN_I8 (inner-product int8 direct screen; variants
 * LOADS, LDS, MFMA, FULL, FULL_MS, FULL_PRIO, FULL_MS_PRIO) or VS_SCREEN_NATIVE (bf16 direct
 * screen; LOADS, MFMA, FULL).  `reps` launches back to back, each between its own HIP events:
 * ms[r] = launch r's duration; stamps[(r * G + b) * 4 + {0,1,2,3}] = workgroup b's s_memtime at the
 * loop's start and end, and its s_memrealtime (100 MHz) at the same points (host array of
 * reps * 256 * 4); *G_out = the launch's workgroups.  Synchronises. */
/* The K-step schedule of the int8 inner-product direct screen (K1), process-wide: 0 = one barrier at
 * the head of every K-step; 1 (default) = the mid-step barrier.  The same keys,
 * survivors and results under either schedule. */
int vs_set_k1_schedule(int32_t schedule);
int vs_k1_schedule(void);
/* The int8 screen's query credit, process-wide: 1 (default) = a query whose own int8 rounding error is
 * below the share every row's bound carries for it gets the difference back, so its exact refine
 * scores fewer rows; 0 = no credit.  Both margins are proven: the same results under either. */
int vs_set_i8_query_credit(int32_t on);
int vs_i8_query_credit(void);
enum {
    VS_K1P_LOADS = 0,        /* corpus loads + query LDS-DMAs + the per-K-step barriers */
    VS_K1P_LDS = 1,          /* + the query-fragment LDS reads */
    VS_K1P_MFMA = 2,         /* + the MFMAs (no tile epilogue) */
    VS_K1P_FULL = 3,         /* the whole loop with the epilogue's bound test (the product's schedule) */
    VS_K1P_FULL_MS = 4,      /* the same under the mid-step-barrier schedule */
    VS_K1P_FULL_PRIO = 5,    /* FULL with static priority 1 for waves 4-7 */
    VS_K1P_FULL_MS_PRIO = 6  /* FULL_MS with static priority 1 for waves 4-7 */
};
int vs_k1_probe(vs_index* index, const float* q_dev, int64_t nq, int32_t screen, int32_t variant,
                int32_t zero_queries, int32_t reps, void* stream, float* ms, unsigned long long* stamps,
                int32_t* G_out);
int vs_timing_fetch(vs_index* index, float* ms, int cap, int* kernel_kind);
int64_t vs_uncertified_count(vs_index* index);   /* first-pass certificate failures; synchronises */
/* queries answered by the exact full scan (no bounded screen could certify them; see
 * vs_search_device_exact); synchronises */
int64_t vs_full_scan_count(vs_index* index);
/* stored rows the adaptive exact refine (behind the int8 screen and the native MFMA first passes) has
 * scored so far, over all queries; synchronises */
int64_t vs_refine_rows_count(vs_index* index);
/* pinned host bytes the index holds for vs_search's query / result staging (all contexts); each
 * context stages at most 8 MiB and loops over query chunks beyond that */
int64_t vs_host_staging_bytes(vs_index* index);
/* HBM bytes the process holds in library workspaces right now (every index, context, selector
 * scratch and graph; the stored rows and their screen copies are not counted): back at its earlier
 * value once the objects made since are destroyed */
int64_t vs_device_bytes_live(void);
/* HBM bytes the screen copies hold beyond the stored rows (VS_SCREEN_I8: int8 codes, per-row scale |
 * error norm); 0 for native screens */
int64_t vs_screen_copy_bytes(vs_index* index);
/* the screen's state, up to `cap` doubles: [0] screen, [1] group residuals in use, [2] groups coded
 * against a mean, [3] max ||mu_g||, [4] max ||x_hat|| of the int8 codes, [5] max row error norm,
 * [6] int8 union log2 depth, [7] searches still routed to the native screen, [8] native seed log2
 * depth (the screen-health feedback described at vs_search_device_exact); synchronises */
#define VS_SCREEN_STATE_N 9
int vs_screen_state(vs_index* index, double* out, int cap);

/* ==== id selectors: exact filtered search on the flat index =================================
 * The product rarely wants "the k nearest photos": it wants the k nearest of a year, or among the
 * paths the keyword store returned.  The reference cannot say that to its index, so it inflates
 * candidate_k, searches unfiltered and throws most of the answer away (core/searcher.py:771-820
 * _calculate_candidate_k, :887 the search, :573-603 _filter_by_time, :931-936 es_filtered_paths,
 * :1165-1211 the relaxation rounds that repeat it).  faiss has the missing call --
 * index.search(q, k, params=SearchParameters(sel=IDSelectorBitmap(n, bitmap))), honoured by
 * IndexFlat -- and these entries are that call made exact.
 *
 * vs_sel_create stands for faiss.IDSelectorBitmap(n, bitmap): id i is allowed iff
 * (bitmap[i >> 3] >> (i & 7)) & 1 (np.packbits(mask, bitorder="little")).  The selector covers rows
 * [0, n_sel), n_sel = the index's ntotal at creation: nbytes < ceil(n_sel / 8) is VS_ERR_ARG, bits
 * at or past n_sel are ignored, rows added later are not selected, and after vs_reset (or a
 * vs_remove_ids that removed a row) the selector is stale (searching with it is VS_ERR_ARG).  Creation uploads the bitmap and compacts it once to
 * an ascending id list on the device; the selector is then reused across searches (the searcher's
 * relaxation rounds repeat one filter).  It takes the index's shared lock, as searches do. */
typedef struct vs_sel vs_sel;
int vs_sel_create(vs_index* index, const uint8_t* bitmap, int64_t nbytes, vs_sel** out);
void vs_sel_destroy(vs_sel* sel);
int64_t vs_sel_count(const vs_sel* sel);   /* m: allowed rows */
/* faiss index.search(q, k, params=SearchParameters(sel=...)) on an IndexFlat: per query the exact
 * top-k among the allowed rows under the canonical fp64 score -- order, tie rule (lower id) and
 * D = (float)S as vs_search; with m allowed rows and k > m the slots past m hold -1 / -+FLT_MAX;
 * k is limited as in vs_search.  Host buffers, staged as vs_search stages them. */
int vs_search_sel(vs_index* index, const vs_sel* sel, const float* q, int64_t nq, int32_t k, float* D, int64_t* I);
/* Two tiers answer a filtered search, with identical bits.  SCAN: the exact streaming scan of the
 * allowed rows alone (nq * m rows gathered).  OVERFETCH: the exact unfiltered search at
 * k' ~ 1.5 k ntotal / m, filtered on the device; a query whose k' entries hold fewer than k allowed
 * rows (and k' < ntotal) is re-answered by the scan -- no query is returned from an unproven
 * prefix.  AUTO (default) picks the scan for 1-2 queries, selective filters and k' past the limit. */
#define VS_SEL_AUTO 0
#define VS_SEL_SCAN 1
#define VS_SEL_OVERFETCH 2
int vs_set_sel_mode(vs_index* index, int mode);
/* the last filtered search on this handle, up to `cap` (4) values: {m, tier taken (VS_SEL_SCAN /
 * VS_SEL_OVERFETCH), k' (0 for the scan), queries re-answered by the scan} */
int vs_sel_last_stats(vs_index* index, int64_t* out, int cap);

/* ==== row removal ============================================================================
 * faiss IndexFlat::remove_ids(IDSelectorBitmap(n, bitmap)): bit i set = remove row i.  Surviving
 * rows keep their order and take ids 0..ntotal'-1.  *n_removed (may be NULL) = rows removed.
 * The reference never calls it -- its indexer only appends (core/indexer.py:763), its searcher drops
 * hits whose file is gone after the search (core/searcher.py:948, :1142) and the only cure is the
 * full rebuild of force_rebuild (core/indexer.py:667-700) -- but its metadata list is indexed by
 * faiss id, which is exactly the shift this call makes.
 *
 * After the call the index is indistinguishable, through every entry point, from one built by
 * vs_add of the surviving rows in order (the stored rows, their norms and the int8 screen copy are
 * compacted in HBM: DESIGN.md §7e).  The bitmap has vs_sel_create's layout: nbytes <
 * ceil(ntotal / 8) is VS_ERR_ARG, bits at or past ntotal are ignored.  A call that removes nothing
 * changes and invalidates nothing.  One that removes a row makes every selector and every vs_hnsw
 * made before it stale (VS_ERR_ARG when used, as after vs_reset).  vs_capacity never changes; with
 * every row removed ntotal is 0.  The call takes the exclusive lock and waits for the device
 * (searches queued by the device API included) before the first row moves.  Its bounce buffer is
 * allocated before anything moves (VS_ERR_OOM leaves the index untouched), is counted in
 * vs_device_bytes_live and is freed before the call returns. */
int vs_remove_ids(vs_index* index, const uint8_t* bitmap, int64_t nbytes, int64_t* n_removed);
/* process-wide: bytes of the bounce buffer a removal may hold (default 256 MiB, floor one row tile:
 * any smaller value, down to 1, means one tile; < 1 is VS_ERR_ARG) */
int vs_set_remove_staging_bytes(int64_t bytes);

/* ==== range search: every row within a score radius ==========================================
 * faiss IndexFlat::range_search(x, radius) -> (lims, D, I).  The reference cuts a guessed top-k at
 * score floors (core/searcher.py:822-843, over the candidate list of :771-820); this call returns
 * exactly the rows that pass the floor, however many there are.
 *
 * For query q with radius r_q (fp32, one per query) and a row of canonical fp64 score S (as
 * vs_search defines it), D = (float)S: the row is returned iff D > r_q (inner product) or D < r_q
 * (L2, squared distance) -- strict, as faiss, and on the fp32 value the caller sees, so a row is
 * returned exactly when vs_search would report a D that satisfies it.  Each query's rows come best
 * first under vs_search's total order (S, then the lower id): a range result equals the first
 * `count` entries of vs_search(k >= count).  radius -inf (IP) / +inf (L2) returns every row; a NaN
 * radius is VS_ERR_ARG; nq = 0 gives lims = {0}; an empty index gives all-zero lims.
 *
 * The result is an owned object (faiss's RangeSearchResult); its size depends on the data, so the
 * call synchronises.  max_total > 0 caps lims[nq]: beyond it the call is VS_ERR_ARG, the message
 * names the count needed and *out is untouched; <= 0 = no cap.  sel may be NULL; with a selector the
 * rules of vs_search_sel hold (a stale selector is VS_ERR_ARG, rows added later are not selected). */
typedef struct vs_range_result vs_range_result;
int vs_range_search(vs_index* index, const vs_sel* sel, const float* q, int64_t nq, const float* radius,
                    int64_t max_total, vs_range_result** out);
const int64_t* vs_range_lims(const vs_range_result* r);   /* nq + 1 */
const float* vs_range_D(const vs_range_result* r);        /* lims[nq] */
const int64_t* vs_range_I(const vs_range_result* r);      /* lims[nq] */
int64_t vs_range_nq(const vs_range_result* r);
void vs_range_free(vs_range_result* r);
/* Two tiers answer a range search, with identical bits.  SCAN (every dtype and metric, any nq, and
 * the only tier with a selector): the exact streaming scan, every row scored canonically.  SCREEN
 * (bf16 / f16 rows, blocks of 9..256 queries, no selector): the native MFMA screen started at the
 * key of r_q lowered by the screen's proven margin, so its survivors are a superset of the answer;
 * they are scored exactly and tested.  A query whose survivor list a workgroup had to cut is
 * re-answered by the scan -- no query is returned from a list that may be incomplete.  AUTO
 * (default): SCREEN where it applies, otherwise SCAN.  The int8 screen setting (vs_set_screen) does
 * not apply to range searches: they always screen the stored rows. */
#define VS_RANGE_AUTO 0
#define VS_RANGE_SCAN 1
#define VS_RANGE_SCREEN 2
int vs_set_range_mode(vs_index* index, int mode);
/* the last range search on this handle, up to `cap` (4) values: {total results, tier taken for the
 * batch (VS_RANGE_SCREEN if any block was screened), queries re-answered by the scan after a screen
 * overflow, queries whose segment (longer than 4096 rows) was sorted on the host} */
int vs_range_last_stats(vs_index* index, int64_t* out, int cap);

/* ==== queries taken from stored rows ==========================================================
 * "What looks like this photo" and "which photos are near-duplicates" ask the index about rows it
 * already holds.  The reference reconstructs the row to a Python list, searches max(k + 1, 5 k) rows
 * and throws its own photo out by path afterwards (core/searcher.py:1751-1814 search_by_image_path);
 * its _deduplicate_results merges equal paths only.  In these two calls the queries never leave the
 * device: query i is the stored value of row ids[i] exactly as vs_reconstruct returns it (fp32, exact
 * for every dtype, not normalised again), gathered in HBM.  ids may repeat and come in any order; an
 * id outside [0, ntotal) is VS_ERR_ARG, checked before anything is launched (so with an empty index
 * only n = 0 is legal).  Both calls take the shared lock, as searches do.
 *
 * self_mode says what becomes of the query's own row:
 *   VS_SELF_KEEP   the result is bit-equal to vs_search (sel NULL) / vs_search_sel / vs_range_search
 *                  on those vectors.
 *   VS_SELF_DROP   the same, with the entry whose id is ids[i] removed -- by id, not by position: a
 *                  duplicate with a lower id scores the same as the row itself and comes first.
 *                  vs_search_rows runs the search at min(k + 1, ntotal); the entry holding ids[i] is
 *                  taken out and the rest moves up; if the row itself is not among the k + 1 (inner
 *                  product over unnormalised rows; a row sel does not allow) the last entry goes
 *                  instead, i.e. the first k stand unchanged; the tail is padded with -1 / -+FLT_MAX as
 *                  vs_search pads it.  k + 1 is therefore what vs_search's limit applies to.
 *   VS_SELF_ABOVE  (vs_range_search_rows only; VS_ERR_ARG for vs_search_rows) only rows with id >
 *                  ids[i] are returned: in a self-join every pair then comes exactly once, as
 *                  (lower id -> higher id), and the scan reads only the rows that can still pass.
 *
 * vs_search_rows: D, I host n x k, as vs_search / vs_search_sel (sel may be NULL); n = 0 returns at
 * once; a stale selector is VS_ERR_ARG; vs_sel_last_stats reports as for vs_search_sel.
 * vs_range_search_rows: radius holds n values; ids NULL = rows 0..n-1, and n must then equal ntotal
 * (the whole-corpus self-join); the removed rows are never counted, so max_total, the error that
 * names the count and vs_range_last_stats see the filtered answer.  n = 0, a NaN radius, a stale
 * selector, max_total and the owned result behave as in vs_range_search. */
enum { VS_SELF_KEEP = 0, VS_SELF_DROP = 1, VS_SELF_ABOVE = 2 };
int vs_search_rows(vs_index* index, const vs_sel* sel, const int64_t* ids, int64_t n, int32_t k, int32_t self_mode,
                   float* D, int64_t* I);
int vs_range_search_rows(vs_index* index, const vs_sel* sel, const int64_t* ids, int64_t n, const float* radius,
                         int32_t self_mode, int64_t max_total, vs_range_result** out);

/* ==== k-means over stored rows ================================================================
 * "Sort these photos into k visual groups" and "train an IVF's coarse quantizer on what the index
 * holds": faiss::Clustering / faiss.Kmeans (the family of IndexFlat and IndexIVFFlat, faiss-cpu,
 * requirements.txt:5) over rows that stay in HBM.  The reference has no such call.
 *
 * Members: rows 0..ntotal-1 (m = ntotal), or with a selector its allowed rows (m = vs_sel_count; a
 * stale selector is VS_ERR_ARG).  A member's point is its stored value exactly as vs_reconstruct
 * returns it, not normalised again.  metric is the ASSIGNMENT metric (VS_METRIC_IP / VS_METRIC_L2,
 * -1 = the index's own): unit-norm cosine stores cluster properly under L2.
 *
 * Assignment pass t = 0, 1, ...: every member goes to its exact best centroid under the canonical
 * fp64 score S (oracle/vs_oracle.c), ties to the lower centroid id; the centroids are the fp32 values
 * as given.  changed[t] = members whose label differs from pass t - 1 (changed[0] = m);
 * objective[t] = the fp64 sum of the members' S in pass t (summation order unspecified).  A pass
 * t >= 1 with changed[t] == 0 ends the call (a fixed point), as does pass t == niter; otherwise
 * update t runs and pass t + 1 follows.  *iters_done = updates run; entries of objective / changed
 * past the last pass are left untouched.  labels, D and counts describe the last pass, i.e. they are
 * consistent with the returned centroids.  niter = 0 is "assign the stored rows to these centroids".
 *
 * Update (reproducible to the bit): a cluster's members in ascending id are cut into segments of
 * VS_KMEANS_SEG consecutive members (the last one shorter); a segment's partial starts at +0.0 and
 * adds its members' values, widened to fp64, one after the other; the cluster's sum starts at +0.0
 * and adds the partials in segment order; the centroid is (float)(sum / (double)count) per column.
 * No FMA, no reassociation.  An empty cluster keeps its centroid.  The result is a pure function of
 * the inputs: it does not depend on the staging size, streams or launch geometry.
 *
 * k < 1, k > m, niter < 0, a bad metric, null centroids or null labels are VS_ERR_ARG, checked
 * before anything is launched (centroids untouched); with m = 0 only k < 1 (and those not about m)
 * fail: the call writes counts = 0, objective[0] = 0, changed[0] = 0, *iters_done = 0.  The call
 * takes the shared lock and synchronises.  Its workspace -- the temporary centroid index's search
 * contexts, the gathered query chunk (vs_set_kmeans_staging_bytes: process-wide, default 256 MiB,
 * floor one 256-row block: any smaller value, down to 1, means one block; < 1 is VS_ERR_ARG), the
 * labels, the member order and the partials -- is counted in vs_device_bytes_live and freed before
 * the call returns. */
#define VS_KMEANS_SEG 256
int vs_kmeans(vs_index* index, const vs_sel* sel, int32_t k, int32_t niter, int32_t metric,
              float* centroids,      /* host k x d fp32: in = initial, out = final */
              int64_t* labels,       /* host m: cluster of each member, members in ascending id */
              float* D,              /* host m: (float)S of the member against its centroid; may be NULL */
              int64_t* counts,       /* host k: members per cluster under `labels`; may be NULL */
              double* objective,     /* host niter + 1; may be NULL */
              int64_t* changed,      /* host niter + 1; may be NULL */
              int32_t* iters_done);  /* updates performed; may be NULL */
int vs_set_kmeans_staging_bytes(int64_t bytes);
/* measurement hook (scripts/kmeans_timing.py): the last vs_kmeans call of the process, up to `cap` (5)
 * values: ms in assignment, in grouping (labels, sort, the host's segment list) and in the update
 * kernels (HIP events on the call's stream, summed over its passes), passes run, updates run */
int vs_kmeans_last_times(double* out, int cap);

/* ==== diversified search ======================================================================
 * "The best k results, one per group of look-alikes": cameras shoot bursts, and a library that holds
 * twelve frames of one moment answers a query with ten frames of the same wave.  The reference's
 * _deduplicate_results (core/searcher.py:242) merges equal paths only, and its relaxation and expansion
 * rounds (core/searcher.py:1157-1211, :1352-1458) re-search with a larger candidate_k to fill the page
 * back up.  vs_search_diverse answers each query q with a suppression radius r_q (fp32, one per query)
 * exactly, on the device, at any depth.
 *
 * Members: every stored row (sel NULL), or the rows the selector allows; a stale selector is
 * VS_ERR_ARG and rows added after the selector was made are not members (the rules of vs_search_sel).
 * Ranking: the members in vs_search's total order for q -- canonical fp64 score S, then the lower id.
 * Near: rows a and b are near iff (float)S(a, b) passes r_q strictly (inner product D > r, L2 D < r),
 * S(a, b) the canonical score of the two stored values as vs_reconstruct returns them.  This is the
 * predicate of vs_range_search_rows: b is near a exactly when that call with ids = {a}, radius = r
 * returns b.  The relation is symmetric bit for bit and NOT transitive, so the order of the walk is
 * part of the contract:
 * Walk: go through the ranking best first; a row is accepted iff it is near no row accepted before
 * it, otherwise it is hidden under the earliest-accepted row it is near; the walk ends with the k-th
 * acceptance or with the ranking.
 *
 * Outputs (host): D, I (nq x k) the accepted rows in acceptance order, D the value vs_search reports
 * for the row, unfilled slots -1 / -+FLT_MAX; hidden (int32 nq x k, may be NULL) the rows hidden under
 * each accepted row among the rows examined, unfilled slots 0; examined (int64 nq, may be NULL) the
 * rows of the ranking the walk looked at: the rank of the k-th accepted row plus one, or the member
 * count when the ranking ran out.  sum(hidden[q]) + accepted[q] == examined[q].
 *
 * r = +inf (inner product) / -inf (L2): nothing is near, the result is bit-equal to vs_search /
 * vs_search_sel.  r = -inf / +inf: everything is near, only the top row is returned and examined is the
 * member count.  A NaN radius, k <= 0, k beyond vs_search's limit (3276) and null q / radius / D / I
 * are VS_ERR_ARG, checked before anything is launched; nq = 0 returns at once; an empty index or a
 * selector that allows nothing gives all padding and examined = 0.  The walk holds a stored row in
 * LDS as an fp64 query: d > 14336 is VS_ERR_ARG.  Shared lock, one leased context, the call
 * synchronises (the shape of vs_search_rows).
 *
 * The accepted list is prefix-stable -- walking deeper only appends -- so a walk over the first L rows
 * of the ranking yields an exact prefix of the answer.  Every query is exact; the list lengths below
 * change the work, never the bits: (1) the exact top-L0 of every query, L0 = min(first, members),
 * walked on the device; (2) queries with fewer than k accepted rows whose list was shorter than the
 * member set are re-searched at 4 L, up to min(limit, members), and walked again; (3) a query still
 * short gets its whole ranking (the range-search scan with an infinite radius), walked by the same
 * kernel -- thousands of identical embeddings at the top of a ranking are still answered.  Tier 3's
 * lists are counted in vs_device_bytes_live and freed before the call returns. */
int vs_search_diverse(vs_index* index, const vs_sel* sel, const float* q, int64_t nq, int32_t k,
                      const float* radius, float* D, int64_t* I, int32_t* hidden, int64_t* examined);
/* list lengths the walk is fed (tests; results are the same bits under every setting):
 * first = 0 -> max(4 k, 64), limit = 0 -> vs_search's k limit; 1 <= first <= limit <= that limit */
int vs_set_diverse_depth(vs_index* index, int32_t first, int32_t limit);
/* last call on the handle, up to cap (5): {queries, complete after the first list, complete after a
 * deeper list, answered from the full ranking, longest list walked} */
int vs_diverse_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/diverse_timing.py): the last call on the handle, up to cap (6): ms of
 * HIP-event time {list search, walk} of tier 1, of tier 2 and of tier 3 ({ranking, walk}) */
int vs_diverse_last_times(vs_index* index, double* out, int cap);

/* ==== grouped search ==========================================================================
 * "The best k days for this query, 3 photos of each": rows that belong together by a key -- a shooting
 * day, a folder, an event, a person, a file hash -- collapsed into one result.  The reference merges
 * equal paths after over-fetching candidate_k rows (_deduplicate_results, core/searcher.py:242) and
 * re-searches to fill the page back up (:1157-1211, :1352-1458); Milvus group_by_field, Qdrant
 * search_groups and Elasticsearch collapse + inner_hits are this call, faiss has none.
 *
 * Group keys.  vs_groups_create takes n host int64 keys, one per row; n must equal vs_ntotal
 * (VS_ERR_ARG otherwise; keys may be NULL when n = 0).  Rows with the same non-negative key form a
 * group; a row with a negative key is a group of its own (an ungrouped photo).  Rows added after
 * creation belong to no group and are no members of a grouped search (the selector's n_sel rule); after
 * vs_reset, or a vs_remove_ids that removed a row, the object is stale (using it is VS_ERR_ARG, the
 * generation check of vs_sel).  Creation sorts the keys on the host and uploads once -- per row a dense
 * group index in ascending key order, per group its key and size, per ungrouped row its key -- and the
 * object is reused across searches.  Shared lock; its HBM is counted in vs_device_bytes_live until
 * vs_groups_destroy.  vs_groups_count: distinct non-negative keys; vs_groups_rows: rows covered. */
typedef struct vs_groups vs_groups;
int vs_groups_create(vs_index* index, const int64_t* keys, int64_t n, vs_groups** out);
void vs_groups_destroy(vs_groups* groups);
int64_t vs_groups_count(const vs_groups* groups);
int64_t vs_groups_rows(const vs_groups* groups);
/* Members: the rows the groups object covers, with a selector (may be NULL) those of them it allows;
 * the rules of vs_search_sel hold (a stale selector is VS_ERR_ARG, rows added later are not selected).
 * Ranking: the members in vs_search's total order for q -- canonical fp64 score S, then the lower id.
 * Answer: the groups ordered by their best member (first appearance in the ranking), the first k of
 * them, and of each its best group_size (g) members in ranking order.
 *
 * Outputs (host): keys_out (int64 nq x k) the group's key, for an ungrouped row its negative key as
 * given; D, I (nq x k x g) the members, D = (float)S exactly as vs_search reports it; found (int32
 * nq x k, may be NULL) the members returned for the group, min(g, members of the group); sizes (int64
 * nq x k, may be NULL) the members of the group under the selector (1 for an ungrouped row).  A group
 * slot past the last group has found 0, sizes 0, keys_out INT64_MIN and every I / D entry padded as
 * vs_search pads (-1 / -+FLT_MAX); member slots past found are padded the same way.
 *
 * With all keys negative, or all distinct, and g = 1, I[:, :, 0] and D[:, :, 0] are bit-equal to
 * vs_search / vs_search_sel at the same k; with all keys equal the one group holds the first g entries
 * of vs_search(q, g).
 *
 * k < 1, group_size < 1, k * group_size beyond vs_search's k limit (3276) or beyond the depth limit
 * below, null q / keys_out / D / I, groups of another index and stale groups are VS_ERR_ARG, checked
 * before anything is launched; nq = 0 returns at once; an empty member set gives all padding.  Shared
 * lock, one leased context, the call synchronises (the shape of vs_search_diverse).
 *
 * No query ranks its whole member set.  target = min(k, groups with a member); a walk over a list that
 * is a prefix of the ranking identifies groups in their true order, so it is complete once it holds
 * target groups with min(g, members of the group) rows each, or once the list holds every member.
 * (1) the exact top-L0 of every query, L0 = min(first, limit, members), walked on the device; (2) the
 * queries not complete re-searched at 4 L up to min(limit, members) and walked again; (3) restricted
 * rounds, one query at a time: the member set is cut down on the device to the rows that can still
 * matter -- the rows of identified groups that are short of members and, while fewer than target groups
 * are identified, the rows of groups not yet seen -- the filtered search's own road ranks the first
 * min(limit, rows left) of them, the walk runs again and the host merges (an identified group's new
 * list extends its old one; new groups follow in their order of appearance).  Every round completes or
 * identifies at least one group because k * group_size <= limit.  The depths change the work, never
 * the bits.  The rounds' scratch is counted in vs_device_bytes_live and freed before the call returns. */
int vs_search_groups(vs_index* index, const vs_groups* groups, const vs_sel* sel, const float* q, int64_t nq,
                     int32_t k, int32_t group_size, int64_t* keys_out, float* D, int64_t* I, int32_t* found,
                     int64_t* sizes);
/* list lengths the walk is fed (tests; the same bits under every setting): first = 0 -> max(4 k g, 64),
 * limit = 0 -> vs_search's k limit; 1 <= first <= limit <= that limit */
int vs_set_group_depth(vs_index* index, int32_t first, int32_t limit);
/* last call on the handle, up to cap (6): {queries, complete after the first list, complete after a
 * deeper list, finished by restricted rounds, restricted rounds run in total, longest list walked} */
int vs_group_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/groups_timing.py): the last call on the handle, up to cap (8): ms of
 * HIP-event time {list search, walk} of tier 1, of tier 2 and of the restricted rounds (their list
 * search = building the restricted set, its compaction and the scan), then the parts of that last
 * search spent building the restricted set and compacting it */
int vs_group_last_times(vs_index* index, double* out, int cap);

/* ==== adjusted search ==========================================================================
 * "Rank by the vector score mixed with a keyword score and a metadata boost": the reference fuses the
 * vector score of its candidate_k vector hits with the keyword store's score and multiplies by a
 * metadata boost (core/searcher.py:925-988, _compute_metadata_boost :435-449); a photo with a strong
 * keyword hit just outside the candidate list is lost.  Per row the fused score is an affine function
 * of the vector score, A = scale_row * S + bias_row: Elasticsearch knn + boost / function_score,
 * Milvus's boost ranker, Qdrant's score-boosting formula; faiss has no such call.  Only the index sees
 * the rows outside a candidate list, so only the index can rank by A exactly.
 *
 * The adjustment.  vs_adjust_create (dense): host fp32 scale[n] and bias[n], either may be NULL (all 1 /
 * all 0); n must equal vs_ntotal.  vs_adjust_create_sparse: m entries (ids, scale, bias), scale / bias
 * may be NULL alike; the ids are distinct and in [0, ntotal), in any order; every other row is plain.
 * A row is plain iff its (scale, bias) is exactly (1.0f, +-0.0f); the others are adjusted, and
 * vs_adjust_count returns how many there are (m_adj); vs_adjust_rows: rows covered.  scale must be
 * finite and >= 0, bias finite: anything else, a NaN included, is VS_ERR_ARG, checked before any upload.
 * Rows added later are no members; after vs_reset, or a vs_remove_ids that removed a row, the object is
 * stale (the generation check of vs_sel / vs_groups).  The object is reused across searches.  Shared
 * lock; its HBM -- fp32 scale[n] and bias[n], the ascending id list of the adjusted rows, the extrema
 * smin, smax, bmin, bmax over the covered rows -- is counted in vs_device_bytes_live until
 * vs_adjust_destroy. */
typedef struct vs_adjust vs_adjust;
int vs_adjust_create(vs_index* index, const float* scale, const float* bias, int64_t n, vs_adjust** out);
int vs_adjust_create_sparse(vs_index* index, const int64_t* ids, const float* scale, const float* bias, int64_t m,
                            vs_adjust** out);
void vs_adjust_destroy(vs_adjust* adjust);
int64_t vs_adjust_count(const vs_adjust* adjust);
int64_t vs_adjust_rows(const vs_adjust* adjust);
/* Members: the rows the adjustment covers, with a selector (may be NULL) those of them it allows, under
 * the rules of vs_search_sel.
 * Adjusted score: A = fl64(fl64((double)scale * S) + (double)bias), S the canonical fp64 score: two
 * rounded fp64 operations, no FMA.  A plain row has A == S bit for bit.
 * Ranking: the members by A in the metric's direction (inner product descending, L2 ascending -- for L2 a
 * bonus is a negative bias), ties to the lower id.
 * Outputs (host, nq x k): D = (float)A, I = the row ids, D_raw (may be NULL) = (float)S, the value
 * vs_search reports for that row; padded as vs_search pads.
 * With every row plain the result is bit-equal to vs_search / vs_search_sel; with a uniform (s, 0), s a
 * power of two, the ids are those of vs_search and D is the scaled value.
 *
 * k < 1 or k > 3276, null q / D / I, a stale adjustment or selector and an adjustment of another index
 * are VS_ERR_ARG before anything is launched; nq = 0 returns at once; an empty member set gives all
 * padding.  Shared lock, one leased context, the call synchronises (the shape of vs_search_groups).
 *
 * Tiers (the same bits under each).  All walk the exact top-L plain lists of vs_search, rescoring every
 * entry canonically before A is formed (A is never computed from a rounded score), L = first, then 4 L
 * up to min(limit, members).
 * DIRECT (AUTO takes it iff m_adj + k <= limit): one adjusted scan over the adjusted rows gives their
 * exact top-min(k, m_adj) by A; the walk drops the list's adjusted entries and merges the plain ones with
 * that list.  Complete iff the list held k plain entries or every member: a plain member outside the
 * list is worse in (S, id) than k plain entries inside it, and A == S for those.  A list of k + m_adj
 * always completes.
 * BOUND (AUTO otherwise): no row is scanned directly.  Every member outside a list whose last entry
 * scores S_L has S <= S_L (inner product); the rounded multiply and add are monotone and scale >= 0, so
 * its A <= U = max(fl(fl(smax S_L) + bmax), fl(fl(smin S_L) + bmax)).  Complete iff the k-th best A of
 * the list is strictly greater than U (L2 mirrored: S >= S_L, A >= min(fl(fl(smin S_L) + bmin),
 * fl(fl(smax S_L) + bmin)), strictly less).  Queries open at the limit go to SCAN.
 * SCAN: the streaming exact scan ranking by A over every member, exact for any input -- thousands of
 * rows tied on A included (scale = 0 with a common bias is legal).
 * Forcing DIRECT with m_adj + k > limit is VS_ERR_ARG.  Scratch is counted in vs_device_bytes_live and
 * freed before the call returns. */
int vs_search_adjusted(vs_index* index, const vs_adjust* adjust, const vs_sel* sel, const float* q, int64_t nq,
                       int32_t k, float* D, int64_t* I, float* D_raw);
#define VS_ADJUST_AUTO 0
#define VS_ADJUST_DIRECT 1
#define VS_ADJUST_BOUND 2
#define VS_ADJUST_SCAN 3
int vs_set_adjust_mode(vs_index* index, int mode);
/* list lengths the walk is fed (tests; the same bits under every setting): first = 0 ->
 * k + min(m_adj, max(k, 64)), limit = 0 -> vs_search's k limit; 1 <= first <= limit <= that limit */
int vs_set_adjust_depth(vs_index* index, int32_t first, int32_t limit);
/* last call on the handle, up to cap (7): {queries, complete after the first list, complete after a
 * deeper list, answered by the scan, longest list walked, tier taken (VS_ADJUST_*), m_adj} */
int vs_adjust_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/adjust_timing.py): the last call on the handle, up to cap (6): ms of
 * HIP-event time {list search, walk} of the first list and of the deeper lists, of the direct scan over
 * the adjusted rows and of the full scan (with the walk that reports its rows) */
int vs_adjust_last_times(vs_index* index, double* out, int cap);

/* ==== fused search =============================================================================
 * "One ranking from several embeddings of one request": the reference embeds each alternative wording
 * of a request, searches each one and merges the lists in Python, keeping a photo's higher score
 * (core/searcher.py _maybe_expand_query_results :1352-1458, _maybe_reflect_query_results :1219-1298,
 * _deduplicate_results :242-261).  Milvus hybrid_search over several requests, Qdrant prefetch + fusion
 * and Elasticsearch's multiple knn clauses are this call; faiss has none.  Two rankings: ANY ("matches
 * any of these wordings", a row's best score over the sub-queries) and ALL ("dog and beach", its worst
 * score).  ALL cannot be assembled from per-query top-k lists -- a row good on every concept can be
 * outside each concept's list -- so only the index can rank it exactly.
 *
 * Members: every stored row, with a selector (may be NULL) the rows it allows, under the rules of
 * vs_search_sel (a stale selector is VS_ERR_ARG; rows added after it was made are not selected).
 * Scores: q is host fp32 nq x m x d, fused query a has the sub-queries q[a][0..m).  S_j is the canonical
 * fp64 score of a row with sub-query j, as vs_search defines it; better / worse are the metric's
 * direction (inner product: larger is better, L2: smaller).  VS_FUSE_ANY: F = the best of S_0..S_{m-1};
 * VS_FUSE_ALL: F = the worst.  No arithmetic touches a score: F is bit-equal to one of the S_j.
 * (Sub-query weights are deliberately no part of the call: a rounded multiply can tie rows that are
 * distinct under S_j, which breaks the list argument below.)
 * Ranking: the members by F in the metric's direction, ties to the lower id.
 * Outputs (host): D (nq x k) = (float)F, I (nq x k) = the row ids, which (nq x k, may be NULL) = the
 * lowest j with S_j == F, D_sub (nq x k x m, may be NULL) = (float)S_j for every j.  Padded as
 * vs_search pads; a padded which is -1, padded D_sub entries take the worst value.
 * m = 1 under either mode is bit-equal to vs_search / vs_search_sel with which = 0; ANY equals the host
 * merge of the m lists of vs_search(q_j, k) (union, best score per id, first k by (score, id));
 * permuting the sub-queries changes only which and the order inside D_sub; repeating one changes
 * nothing (which keeps the lower index).
 *
 * m < 1 or m > VS_FUSE_MAX_Q, a mode other than the two, k < 1 or k > min(3276, VS_FUSE_WALK_MAX / m),
 * null q / D / I and a stale selector are VS_ERR_ARG before anything is launched; nq = 0 returns at
 * once; an empty member set gives all padding.  Shared lock, one leased context, the call synchronises
 * (the shape of vs_search_adjusted).  Scratch is counted in vs_device_bytes_live and freed before the
 * call returns.
 *
 * Limits.  The walk kernel ranks at most VS_FUSE_WALK_MAX entries (m lists of L) in LDS, so a list is at
 * most min(3276, VS_FUSE_WALK_MAX / m) long: the bound on k and the default depth limit.  Beside n
 * entries (n rounded up to a power of two, 12 bytes each) the walk holds one sub-query as fp64 in
 * 144 KiB of LDS: d <= 8 * floor((147456 - 12 n) / 64), which is d <= 6144 at n = VS_FUSE_WALK_MAX and
 * d <= 12288 at n <= 4096.  A call whose deepest walk would not fit is VS_ERR_ARG (lower the limit with
 * vs_set_fuse_depth).
 *
 * Tiers (the same bits under each).
 * LISTS: the exact top-L list of every sub-query among the members (one batched search of nq m queries,
 * under the selector where one is given), then a device walk over their union, one workgroup per fused
 * query: every distinct candidate is rescored canonically against all m sub-queries (the staged fp32
 * scores are never used), F, which and the m scores are formed, and the candidates are ranked by
 * (F, id).
 *   ANY is complete at L = min(k, members), the only list it ever needs (the depth settings do not
 *   apply): were a row of the answer with F = S_j outside list j, k members would be better than it
 *   under (S_j, id), and each of those has F at least as good, an equal F only at a lower id.
 *   ALL takes L = first, then 4 L up to min(limit, members).  A member outside every list is, for every
 *   j, no better than list j's last entry S_{j,L}, so its F is no better than U, the worst over j of
 *   S_{j,L} (the walk's own rescoring).  Complete iff the lists held every member, or there are at least
 *   k candidates and the k-th best candidate F is strictly better than U.  Queries open at the limit go
 *   to SCAN.
 * SCAN: a streaming scan, exact for any input, ties by the thousand included.  Each workgroup scans its
 * share of the members in ascending id, scores every row against all m sub-queries in one pass over the
 * row, reduces to F and keeps a bounded running top-k under (F, id); the walk then reports which and
 * D_sub of the k winners.
 * AUTO: ANY uses LISTS; ALL uses LISTS, then SCAN for what stays open.  vs_set_fuse_mode forces SCAN, or
 * LISTS with the same fall-through. */
#define VS_FUSE_MAX_Q 8
#define VS_FUSE_WALK_MAX 8192
enum { VS_FUSE_ANY = 0, VS_FUSE_ALL = 1 };
int vs_search_fused(vs_index* index, const vs_sel* sel, const float* q /* host nq x m x d */, int64_t nq,
                    int32_t m, int32_t mode, int32_t k, float* D, int64_t* I, int32_t* which, float* D_sub);
#define VS_FUSE_AUTO 0
#define VS_FUSE_LISTS 1
#define VS_FUSE_SCAN 2
int vs_set_fuse_mode(vs_index* index, int tier);
/* list lengths ALL's walk is fed (tests; the same bits under every setting): first = 0 -> max(4 k, 64),
 * limit = 0 -> min(3276, VS_FUSE_WALK_MAX / m); 1 <= first <= limit <= 3276, and a call cuts both to its
 * own default limit */
int vs_set_fuse_depth(vs_index* index, int32_t first, int32_t limit);
/* last call on the handle, up to cap (6): {fused queries, complete after the first list, complete after
 * a deeper list, answered by the scan, longest list walked, tier taken (VS_FUSE_LISTS / VS_FUSE_SCAN)} */
int vs_fuse_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/fuse_timing.py): the last call on the handle, up to cap (6): ms of
 * HIP-event time {list search, walk} of the first list and of the deeper lists, of the scan and of the
 * walk that reports the scan's rows */
int vs_fuse_last_times(vs_index* index, double* out, int cap);

/* ==== multi-vector search ======================================================================
 * "The trip with mountains, a lake and a campfire": rank groups (an album, a day, a person, a video) by
 * the sum over the sub-queries of the best score any member reaches -- MaxSim, late interaction.  Qdrant
 * multivectors (max_sim), Milvus embedding lists, Weaviate multi-vector and Vespa tensors are this call;
 * faiss has none.  It cannot be assembled from per-concept top-k lists: a group mediocre on every concept
 * can be outside each list and still win the sum.
 *
 * Queries: q is host fp32 nq x m x d, as vs_search_fused takes it, 1 <= m <= VS_FUSE_MAX_Q.
 * Groups: a vs_groups object under vs_search_groups' rules -- rows with the same non-negative key form a
 * group, a row with a negative key is a group of its own (reported with its key as given), rows added
 * after the object was made are no members, stale groups or groups of another index are VS_ERR_ARG.
 * Members: the covered rows, restricted by sel (may be NULL) under vs_search_sel's rules.  A group with no
 * member under the selector does not exist for the call.
 * Per sub-query best: S_j(row) is the canonical fp64 score, as vs_search defines it.  M_j(g) is the best
 * S_j over the members of g in the metric's direction: a selection, bit-equal to one member's score;
 * I_sub[j] is the lowest member id that attains it.  (Every accumulator starts at +0.0, so no S is -0.0.)
 * Group score: F(g) = ((M_0 + M_1) + ...) + M_{m-1} in fp64, left to right, no contraction.  For L2 this
 * is a sum of smallest distances, and lower is better.
 * Ranking: the groups by F in the metric's direction, ties to the lower group code: grouped groups in
 * ascending key, then the ungrouped rows in row order.
 * Outputs (host): keys_out (int64 nq x k), F (double nq x k: the ranking value, not rounded), D_sub (float
 * nq x k x m, may be NULL) = (float)M_j, I_sub (int64 nq x k x m, may be NULL), sizes (int64 nq x k, may be
 * NULL) = the members of the group under the selector.  Padding as vs_search_groups pads: keys_out
 * INT64_MIN, I_sub -1, D_sub the worst value, F -inf (inner product) or +inf (L2), sizes 0.
 * With m = 1, keys_out, (float)F and I_sub equal vs_search_groups(k, group_size = 1)'s keys, D and I
 * whenever the groups' best scores are distinct; with every key distinct as well it is vs_search.  F is
 * the fp64 sum of the best scores, recomputable from vs_reconstruct'ed rows.  Permuting the sub-queries
 * permutes D_sub / I_sub and may change F only through the order of the additions.
 *
 * m out of range, k < 1 or k > min(3276, VS_FUSE_WALK_MAX / m), null q / keys_out / F, stale or foreign
 * groups or selector are VS_ERR_ARG before anything is launched; nq = 0 returns at once; an empty member
 * set gives all padding.  Shared lock, one leased context, the call synchronises (the shape of
 * vs_search_fused).  Scratch is counted in vs_device_bytes_live and freed before the call returns.  The
 * first call with a groups object builds its member lists (the covered rows by (group, id) and their
 * offsets, 4 bytes per row + 8 per group); they live until vs_groups_destroy and are counted too.
 *
 * Tiers (the same bits under each: both end in the same walk kernel).
 * LISTS: the exact top-L list of every sub-query among the members, then a device walk, one workgroup per
 * query: the groups the lists touch are its candidates, each is scored member by member against all m
 * sub-queries, and the candidates are ranked by (F, code).  L = first, then 4 L up to min(limit,
 * members).  A group no list touches has every M_j no better than list j's last entry S_{j,L}; rounding
 * and addition are monotone, so its F is no better than U = ((S_{0,L} + S_{1,L}) + ...).  Complete iff
 * the lists held every member, or there are at least k candidates and the k-th best F is strictly better
 * than U.  A query whose candidate groups hold more than walk_rows rows goes to SCAN at once (a few huge
 * groups otherwise make one workgroup score half the corpus; deeper lists only add candidates), and so does
 * an open query whose walk went through more than walk_rows / 4 rows (its next lists are four times as long).  Queries
 * open at the limit go to SCAN.  Beside the lists a walk keeps 12 m + 8 bytes of scratch per list entry and
 * query, about 64 MiB per launch (queries beyond that go in further launches).
 * SCAN: a streaming scan over the members scores every row against all m sub-queries in one pass and keeps,
 * per (query, sub-query, group), the maximum of an order-preserving 64-bit image of S in a device table
 * (blocks of queries bounded by vs_set_maxsim_staging_bytes); a rank kernel forms F per group and keeps
 * the k best; the walk then reports those groups.
 * AUTO: LISTS, then SCAN for what stays open.  vs_set_maxsim_mode forces SCAN, or LISTS with the same
 * fall-through. */
int vs_search_maxsim(vs_index* index, const vs_groups* groups, const vs_sel* sel /* may be NULL */,
                     const float* q /* host nq x m x d */, int64_t nq, int32_t m, int32_t k, int64_t* keys_out,
                     double* F, float* D_sub, int64_t* I_sub, int64_t* sizes);
#define VS_MAXSIM_AUTO 0
#define VS_MAXSIM_LISTS 1
#define VS_MAXSIM_SCAN 2
int vs_set_maxsim_mode(vs_index* index, int tier);
/* list lengths the walk is fed and the row cap of one walk (the same bits under every setting): first = 0
 * -> max(4 k, 64), limit = 0 -> min(3276, VS_FUSE_WALK_MAX / m), walk_rows = 0 -> 400 min(nq, 256); 1 <=
 * first <= limit <= 3276, and a call cuts both to its own default limit */
int vs_set_maxsim_depth(vs_index* index, int32_t first, int32_t limit, int64_t walk_rows);
/* bytes of the scan's table per block of queries (process-wide, default 64 MiB; below one query's table
 * it acts as that table) */
int vs_set_maxsim_staging_bytes(int64_t bytes); /* >= 1 */
/* last call on the handle, up to cap (7): {queries, complete after the first list, complete after a deeper
 * list, answered by the scan, longest list walked, tier taken (VS_MAXSIM_LISTS / VS_MAXSIM_SCAN), rows of
 * the candidate groups the answering walks went through} */
int vs_maxsim_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/maxsim_timing.py): the last call on the handle, up to cap (7): ms of HIP-event
 * time {list search, walk} of the first list and of the deeper lists, of the scan, of the rank and of the
 * final walk */
int vs_maxsim_last_times(vs_index* index, double* out, int cap);

/* ==== paged search =============================================================================
 * "Load more": continue a ranking after a cursor row.  Every ranking above stops at k <= 3276; this call
 * returns the k rows that follow a given row of vs_search's ranking, exactly, at any depth, without
 * state on either side (Elasticsearch from/size and search_after, Qdrant offset, Milvus offset and its
 * search iterator, Weaviate after; faiss has none).
 *
 * Members: every stored row, with a selector (may be NULL) the rows it allows, under the rules of
 * vs_search_sel (a stale selector is VS_ERR_ARG; rows added after it was made are not selected).
 * Cursor: after[q] = c >= 0 names a stored row; with S* the canonical fp64 score of row c (the values
 * vs_reconstruct returns) with query q, the cursor is the position (S*, c) in vs_search's total order
 * (score in the metric's direction, then the lower id).  Row c need not be a member -- the selector may
 * disallow it, or it may have been added after the selector was made: the position is defined either way.
 * after[q] = -1 is the position before every row.
 * Answer: the members that rank strictly after the cursor -- a worse S, or an equal S and an id > c -- the
 * first k of them in the total order; D = (float)S, exactly what vs_search reports for the row; padded as
 * vs_search pads (-1, -FLT_MAX / +FLT_MAX).  "Equal" and "worse" are numeric comparisons of doubles, the
 * ones the scans' running top-k uses: +0.0 and -0.0 tie and the id decides.
 * rank[q] (may be NULL): the members at or before the cursor, i.e. the 0-based position, in the members'
 * ranking, of the first returned row; 0 for after = -1, the member count when nothing is left.
 * Identities: after = -1 is bit-equal to vs_search / vs_search_sel; pages chained by "after = the last id
 * of the previous page" concatenate to the members' whole ranking (vs_range_search with an infinite
 * radius), rank of each page being the rows returned so far; a page with fewer than k rows ends it.
 * rank_hint[q] (array may be NULL; -1 = unknown): the caller's guess of rank[q] -- an iterator knows it,
 * the previous rank plus the rows returned.  It changes the work only, never the bits: a wrong hint costs
 * deeper lists or a scan, never a wrong row.
 *
 * k < 1 or k > 3276, null q / after / D / I, after[q] < -1 or >= ntotal (on an empty index only -1 is
 * legal), a stale selector and d > 14336 (the cut kernel stages the query as fp64 in LDS) are VS_ERR_ARG
 * before anything is launched; nq = 0 returns at once; an empty member set gives all padding and rank 0.
 * Shared lock, one leased context, the call synchronises (the shape of vs_search_adjusted).  Scratch is
 * counted in vs_device_bytes_live and freed before the call returns.
 * Not covered: the caller must pass the same query bits on every page of a chain (S* is recomputed from
 * them); ids shift after vs_remove_ids, so a cursor taken before a removal names another row.
 *
 * Tiers (the same bits under each).  The cursor rows are scored first, one wave per query.
 * LISTS: the exact top-L list of every query among the members, then a cut kernel, one workgroup per
 * query, that finds p, the list's entries at or before the cursor.  Rounding to fp32 is monotone, so an
 * entry whose staged D is strictly better (worse) than (float)S* is before (after) the cursor; only the
 * entries with D == (float)S* are rescored canonically and compared by (S, id).  The page is entries
 * p .. p+k-1 as staged and rank = p; complete iff L - p >= k or the list held every member, else the
 * list is re-searched at 4 L up to min(limit, members).  The first list is max(first, rank_hint + k) over
 * the batch's hinted queries when that is within the limit.
 * SCAN: the streaming scan of the members in ascending id with the rows at or before the cursor passed
 * over and counted into rank; exact for any input -- cursors beyond the limit, rows tied with the cursor
 * by the thousand.
 * AUTO: a query whose rank_hint + k exceeds the limit goes straight to SCAN, the others to LISTS; what is
 * open at the limit goes to SCAN.  vs_set_after_mode forces SCAN, or LISTS with the same fall-through
 * (hints beyond the limit are then ignored). */
int vs_search_after(vs_index* index, const vs_sel* sel, const float* q, int64_t nq, int32_t k,
                    const int64_t* after /* host nq */, const int64_t* rank_hint /* host nq, may be NULL */,
                    float* D, int64_t* I /* host nq x k */, int64_t* rank /* host nq, may be NULL */);
#define VS_AFTER_AUTO 0
#define VS_AFTER_LISTS 1
#define VS_AFTER_SCAN 2
int vs_set_after_mode(vs_index* index, int tier);
/* list lengths the cut is fed (tests; the same bits under every setting): first = 0 -> max(4 k, 64),
 * limit = 0 -> 3276 (vs_search's k limit); 1 <= first <= limit <= 3276 */
int vs_set_after_depth(vs_index* index, int32_t first, int32_t limit);
/* last call on the handle, up to cap (6): {queries, complete after the first list, complete after a
 * deeper list, answered by the scan, longest list walked, tier taken (VS_AFTER_SCAN when forced, else
 * VS_AFTER_LISTS: under AUTO the scan's share is the fourth number)} */
int vs_after_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/after_timing.py): the last call on the handle, up to cap (6): ms of HIP-event
 * time {list search, cut} of the first list and of the deeper lists, of the cursor scoring and of the
 * scan */
int vs_after_last_times(vs_index* index, double* out, int cap);

/* ==== facet counts =============================================================================
 * "About 1,240 photos -- 2019 (12), 2020 (40), 2021 (7)": how many members pass a radius, and how they
 * split over a group key, exactly, without producing, ordering or shipping a single row (Elasticsearch
 * count + terms aggregation, Qdrant count + facet, Typesense / Meilisearch facet_by; faiss has none).
 * vs_range_search + a host bincount answers the same question, but appends 12 bytes per passing row,
 * sorts every segment, ships 20 bytes per result and refuses past max_total; this call moves
 * nq x (G + 1) integers.
 *
 * Members: with groups, the rows the groups object covers (rows added later are no members, the rule of
 * vs_search_groups); without groups (NULL), every stored row; with a selector (may be NULL) those of
 * them it allows, under vs_search_sel's rules.  A stale selector, stale groups and groups of another
 * index are VS_ERR_ARG.
 * Predicate: vs_range_search's, exactly.  S the canonical fp64 score, D = (float)S: a member passes iff
 * D > radius[q] (inner product) or D < radius[q] (squared L2) -- strict, on the fp32 value.
 * Outputs, G = vs_groups_count(groups):
 *   counts[q][g], g < G: passing members of the group with the g-th smallest non-negative key (the
 *                        column order is vs_groups_keys');
 *   counts[q][G]:        passing members with a negative key (ungrouped rows), together;
 *   totals[q]:           passing members = the sum of row q of counts.
 * Identities (tests/test_gpu_facet.py holds the call to them):
 *   totals[q] == lims[q + 1] - lims[q] of vs_range_search under the same selector, restricted to the
 *   covered rows; counts[q] == the bincount of the group codes over that call's I; with radius -inf
 *   (inner product) or +inf (L2) counts[q][g] is the group's size under the selector -- the `sizes`
 *   vs_search_groups reports; with the opposite infinity everything is 0.
 *
 * A NaN radius, null q, null radius, null counts with groups (or counts without groups) and both outputs
 * null are VS_ERR_ARG before anything is launched; nq = 0 returns at once; an empty member set gives
 * zeros.  Shared lock, one leased context, the call synchronises (the shape of vs_range_search).
 *
 * Tiers (the same integers under each; vs_set_range_mode applies):
 * SCAN: every dtype and metric, any nq, with or without a selector: the range scan with a histogram in
 * place of the pair buffer.
 * SCREEN: bf16 / f16, blocks of 9..256 queries, no selector: the native MFMA screen started at the
 * radius' key, then the exact refine over the survivors.  A query whose survivor list a workgroup had to
 * cut (drop > thr0) is left alone by the refine and answered by the scan: no query is counted from a
 * list that may be incomplete, no row is counted twice.
 * Histogram forms of the scan (the same integers under each; vs_set_facet_hist):
 * GLOBAL: one 64-bit device atomic per distinct bin among the rows a wave scored in one step;
 * LDS: G + 1 uint32 bins in the workgroup's LDS behind the query, flushed per query -- the non-zero bins
 * only -- with one device atomic each; needs G + 1 <= VS_FACET_LDS_BINS (forcing it past that is
 * VS_ERR_ARG); AUTO: DESIGN §7m.
 *
 * Device memory: the counter table of one query block, nqb x (G + 1) 64-bit counters, bounded by
 * vs_set_facet_staging_bytes (process-wide, default 64 MiB; values below one query's row of counters
 * act as that row): a block takes min(256, bytes / (8 (G + 1))) queries, at least 1; a block of fewer
 * than 9 takes SCAN.  The table is counted in vs_device_bytes_live and freed before the call returns.
 *
 * Not covered: queries taken from stored rows (VS_SELF_*); several radii per query (repeat the query);
 * per-group best rows (vs_search_groups); sums or means of scores (they depend on summation order). */
int vs_range_count(vs_index* index, const vs_groups* groups /* may be NULL */, const vs_sel* sel /* may be NULL */,
                   const float* q, int64_t nq, const float* radius /* host nq */,
                   int64_t* counts /* host nq x (G + 1); NULL iff groups is NULL */,
                   int64_t* totals /* host nq, may be NULL */);
/* the G distinct non-negative keys of a groups object, ascending: the columns of counts */
int vs_groups_keys(const vs_groups* groups, int64_t* out /* host G, ascending */);
#define VS_FACET_HIST_AUTO 0
#define VS_FACET_HIST_LDS 1
#define VS_FACET_HIST_GLOBAL 2
#define VS_FACET_LDS_BINS 8192
int vs_set_facet_hist(vs_index* index, int form);
int vs_set_facet_staging_bytes(int64_t bytes); /* >= 1 */
/* last call on the handle, up to cap (5): {sum of totals, tier taken (VS_RANGE_SCAN / VS_RANGE_SCREEN),
 * queries re-answered by the scan, histogram form the scan took (0: no scan ran), query blocks} */
int vs_facet_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/facet_timing.py): the last call on the handle, up to cap (3): ms of
 * HIP-event time {screen + refine, scan, table readback} */
int vs_facet_last_times(vs_index* index, double* out, int cap);

/* ==== duplicate groups =========================================================================
 * "Which photos are the same shot" -- bursts, re-imports, edited copies -- asks for one label per row: the
 * connected components of "within a radius of each other" (DBSCAN with min_samples = 1, single linkage cut
 * at a radius, the duplicate-cluster step of every deduplication pipeline; faiss has none).
 * vs_range_search_rows(VS_SELF_ABOVE) + a host union-find answers the same question, but a burst of b
 * frames is b (b - 1) / 2 pairs: 12 bytes each in HBM, a sort of every segment, 20 bytes each over PCIe
 * and a refusal past max_total.  This call unites on the device and moves ntotal integers.
 *
 * Members: every stored row, or with a selector (may be NULL) the rows it allows, under vs_search_sel's
 * rules: a stale selector is VS_ERR_ARG, rows added after the selector was made are no members.
 * Edge: members a < b are joined iff vs_range_search_rows(ids = {a}, radius, VS_SELF_ABOVE) under the
 * same selector returns b: S the canonical fp64 score of the two stored values, D = (float)S, and the edge
 * is there iff D > radius (inner product) or D < radius (squared L2) -- strict, on the fp32 value; the
 * predicate of VectorStore.find_duplicates and vs_search_diverse, bit for bit.  One scalar radius: a
 * radius per row would make the relation asymmetric.  A row that is no member carries no edge: a - x - b
 * with x not allowed does not join a and b.
 * Outputs:
 *   labels[i]      the smallest id of the component member i belongs to (a member with no near member is
 *                  its own label); -1 for a row that is no member;
 *   *n_components  distinct non-negative labels, singletons included;
 *   *n_edges       edges, = lims[n] of the VS_SELF_ABOVE self-join over the members.
 * The result is a pure function of the stored rows, the selector and the radius: it does not depend on
 * the tier, the grid or the order in which the device unites.
 * Identities (tests/test_gpu_components.py holds the call to them):
 *   the labels are the components of the pair list of vs_range_search_rows(ids NULL | the allowed ids,
 *   sel, VS_SELF_ABOVE), and n_edges is that call's total; radius -inf (inner product) / +inf (L2) gives
 *   one component -- every member labelled with the lowest member id -- and m (m - 1) / 2 edges for m
 *   members; the opposite infinity gives every member its own label and 0 edges; vs_groups_create(labels)
 *   on an unfiltered result has vs_groups_count == *n_components (the labels are valid keys for
 *   vs_search_groups -- "one result per burst" -- and vs_range_count -- "matches per burst").
 *
 * A NaN radius, null labels with ntotal > 0 and a stale selector are VS_ERR_ARG before anything is
 * launched; an empty index returns at once with both counts 0; a selector that allows nothing gives all
 * -1 and both counts 0.  There is no max_total: nothing grows with the number of pairs.
 * Shared lock, one leased context, the call synchronises (the shape of vs_range_count).
 *
 * Tiers (the same labels and counts under each; vs_set_range_mode applies).  The members in ascending id
 * are the queries, in blocks of 256, gathered on the device from their own rows.
 * SCAN: every dtype and metric, with or without a selector: the range scan over the rows at or above the
 * block's first member (with a selector: over the tail of its id list from the block's first position).
 * SCREEN: bf16 / f16, blocks of 9..256 queries, no selector: the native MFMA screen started at the
 * radius' key, then the exact refine over the survivors.  A query whose survivor list a workgroup had to
 * cut (drop > thr0) is left alone by the refine and answered by the scan.
 *
 * Device memory: the parent array (4 bytes per row), the per-block edge counters (2 KiB per block) and the
 * device labels (8 bytes per row), counted in vs_device_bytes_live and freed before the call returns.
 *
 * Not covered: vs_multi_* across shards (components need the edges between shards); a screen for f32
 * stores.  Neighbour counts per row and core-point DBSCAN (min_samples > 1): "density clusters" below. */
int vs_range_components(vs_index* index, const vs_sel* sel /* may be NULL */, float radius,
                        int64_t* labels /* host ntotal */, int64_t* n_components /* may be NULL */,
                        int64_t* n_edges /* may be NULL */);
/* last call on the handle, up to cap (6): {members, edges, components, tier taken (VS_RANGE_SCAN /
 * VS_RANGE_SCREEN), queries re-answered by the scan after a screen overflow, query blocks} */
int vs_components_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/components_timing.py): the last call on the handle, up to cap (3): ms of
 * HIP-event time {gather + screen + refine, scan, flatten + readback} */
int vs_components_last_times(vs_index* index, double* out, int cap);

/* ==== density clusters =========================================================================
 * Events, faces, scenes: clusters that a stray in-between frame must not fuse.  vs_range_components is
 * single linkage and chains; DBSCAN's core points stop that: a row founds or extends a cluster only if it
 * has at least min_samples rows within the radius, itself included (sklearn.cluster.DBSCAN's convention;
 * Immich's minFaces).  faiss has neither this nor the per-row neighbour count under it.
 *
 * Members, selector and the neighbour relation are vs_range_components': members a < b are neighbours iff
 * vs_range_search_rows(ids = {a}, radius, VS_SELF_ABOVE) under the same selector returns b -- D = (float)S
 * passes the one scalar radius strictly.  A stale selector is VS_ERR_ARG, rows added after the selector are
 * no members, a non-member carries no edge.
 *   degrees[i]  the number of other members that are neighbours of i; -1 for a non-member.  The degrees of
 *               the members sum to 2 * *n_edges.
 *   core        a member with degrees[i] + 1 >= min_samples.  min_samples < 1 is VS_ERR_ARG.
 *   clusters    the connected components of the neighbour relation restricted to the core rows; a cluster's
 *               label is the smallest id of its core rows.
 *   border      a member that is not core and has at least one core neighbour.  It takes the label of its
 *               best core neighbour under vs_search's total order: the greatest D (inner product) or the
 *               smallest (squared L2), D compared as floats (-0.0f and +0.0f tie), ties to the lower core
 *               id.  The choice does not depend on the tier, the grid or the order in which edges are met (it
 *               differs on purpose from sklearn's scan-order rule).  A border row joins one cluster only and
 *               joins no two clusters together.
 *   noise       a member that is neither: label -1.
 *   labels[i]   the cluster's label, -1 for noise and for a non-member.
 *   kinds[i]    VS_DBSCAN_NONE for a non-member, else VS_DBSCAN_NOISE / _BORDER / _CORE.
 *   counts      {clusters, core rows, border rows, noise rows}.
 * Identities (tests/test_gpu_dbscan.py): min_samples = 1 gives vs_range_components' labels with every member
 * core; min_samples = 2 gives its components of two or more members, the singletons noise, no border row;
 * degrees is the bincount of both ends of the VS_SELF_ABOVE pair list.  The labels of an unfiltered call are
 * valid keys for vs_groups_create (noise ungrouped).
 *
 * A NaN radius, min_samples < 1, a null labels / degrees (the required output) with ntotal > 0 and a stale
 * selector are VS_ERR_ARG before anything is launched.  kinds, degrees (of vs_range_dbscan), counts and
 * n_edges may be NULL.  There is no max_total: nothing grows with the number of pairs.  Shared lock, one
 * leased context, the call synchronises.
 *
 * Two passes of vs_range_components' self-join (its tiers, blocks and vs_set_range_mode): pass 1 counts the
 * degrees and each query's edges above; pass 2 unites core rows and offers core rows to their non-core
 * neighbours, skipping the queries -- and whole blocks -- that met no edge in pass 1.  A count is not
 * idempotent, so under the SCREEN tier the overflow flags are read before the refine and every query is
 * answered by exactly one of refine and scan.
 * Device memory, freed before the call returns: 4 B (degrees) per row and 8 B per query slot; vs_range_dbscan
 * adds 4 + 1 + 8 B per row (parent, core, best) and 8 + 1 + 8 B per row of device outputs. */
enum { VS_DBSCAN_NONE = 0, VS_DBSCAN_NOISE = 1, VS_DBSCAN_BORDER = 2, VS_DBSCAN_CORE = 3 };
int vs_range_degrees(vs_index* index, const vs_sel* sel /* may be NULL */, float radius,
                     int64_t* degrees /* host ntotal */, int64_t* n_edges /* may be NULL */);
int vs_range_dbscan(vs_index* index, const vs_sel* sel /* may be NULL */, float radius, int64_t min_samples,
                    int64_t* labels /* host ntotal */, uint8_t* kinds /* host ntotal, may be NULL */,
                    int64_t* degrees /* host ntotal, may be NULL */, int64_t* counts /* 4, may be NULL */,
                    int64_t* n_edges /* may be NULL */);
/* last vs_range_degrees / vs_range_dbscan on the handle, up to cap (12): {members, edges, clusters, core,
 * border, noise, tier taken (VS_RANGE_SCAN / VS_RANGE_SCREEN), pass 1: queries given to the scan after a
 * screen overflow, query blocks; pass 2: the same, query blocks run, queries skipped (no edge in pass 1)} */
int vs_dbscan_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/dbscan_timing.py): the last call on the handle, up to cap (5): ms of HIP-event
 * time {pass 1 gather + screen + refine, pass 1 scan, pass 2 gather + screen + refine, pass 2 scan, labels +
 * readback} */
int vs_dbscan_last_times(vs_index* index, double* out, int cap);

/* ==== score selectors ==========================================================================
 * "Beach, NOT people", "only photos that look like this one", "drop everything near these rejected shots,
 * then cluster the rest": a filter that is itself a vector predicate.  vs_sel_create takes a host bitmap,
 * so such a filter had to go vs_range_search -> ids -> host mask -> vs_sel_create: a pair list the size of
 * the passing rows appended, sorted and shipped, and a max_total.  These calls build the vs_sel on the
 * device: a passing row sets one bit, nothing grows with the number of matches, there is no max_total, and
 * the result is an ordinary vs_sel for every call that takes one (vs_search_sel, vs_search_after,
 * vs_search_groups, vs_search_adjusted, vs_search_fused, vs_search_diverse, vs_range_search, vs_range_count,
 * vs_range_components, vs_kmeans).
 *
 * Members M: rows [0, ntotal) at the time of the call, with a base selector (may be NULL) those it allows,
 * under vs_search_sel's rules (a stale base is VS_ERR_ARG; rows added after the base was made are no members).
 * Predicate: vs_range_search's, bit for bit.  S the canonical fp64 score, D = (float)S: row i passes query j
 * iff D > radius[j] (inner product) or D < radius[j] (squared L2) -- strict, on the fp32 value.  Infinite
 * radii are legal, NaN is VS_ERR_ARG.
 * mode VS_SELQ_ANY: the row passes at least one query; VS_SELQ_ALL: every query.  nq = 0: ANY passes
 * nothing, ALL everything, decided on the host without a scoring kernel.
 * negate != 0: the result is M minus the passing rows.  The result is always a subset of M.
 * The new selector covers the rows present now (n_sel = ntotal), carries the reset generation and goes
 * stale as vs_sel_create's does; its bitmap is zero at and past n_sel, its ids ascend.
 *
 * vs_sel_from_range_rows: the queries are the stored values of rows ids[0, n) (any order, repeats fine),
 * gathered on the device; a row passes its own predicate like any other row (VS_SELF_KEEP).  An id outside
 * [0, ntotal) is VS_ERR_ARG before anything is launched.
 *
 * Tiers (the same bits under each; vs_set_range_mode applies), per block of at most 256 queries:
 * SCAN: every dtype and metric, any nq, with or without a base (with one: over its id list).
 * SCREEN: bf16 / f16, blocks of 9..256 queries, no base: the native MFMA screen started at the radius'
 * key, then the exact refine over the survivors.  A query whose survivor list a workgroup had to cut
 * (drop > thr0) is left alone by the refine and answered by the scan.
 * ANY: every query sets bits in one bitmap.  ALL: each query of a block has a bitmap of its own, ANDed into
 * the accumulator after the block; a block takes min(256, staging bytes / (8 ceil(ntotal / 64))) queries, at
 * least 1 (vs_set_scoresel_staging_bytes, process-wide, default 64 MiB).  Temporaries are counted in
 * vs_device_bytes_live and freed before the call returns.
 *
 * vs_sel_combine: out = a AND b, a OR b, a AND NOT b, or NOT a (b must be NULL).  Both operands belong to
 * `index` and its current generation (else VS_ERR_ARG).  With different n_sel the result covers the larger
 * and the shorter operand reads as zero past its end; VS_SEL_NOT covers a's n_sel.
 * vs_sel_bitmap: the selector's rows as vs_sel_create's bitmap, ceil(n_sel / 8) bytes, the bits at or past
 * n_sel zero; nbytes below that is VS_ERR_ARG.
 *
 * Shared lock, one leased context, the calls synchronise (the shape of vs_sel_create).
 * Not covered: vs_multi_* (build on a one-device copy); IVF and HNSW; device-pointer entry points; weighted
 * combinations of predicates. */
#define VS_SELQ_ANY 0
#define VS_SELQ_ALL 1
int vs_sel_from_range(vs_index* index, const vs_sel* base /* may be NULL */, const float* q /* host nq x d */,
                      int64_t nq, const float* radius /* host nq */, int32_t mode, int32_t negate, vs_sel** out);
int vs_sel_from_range_rows(vs_index* index, const vs_sel* base /* may be NULL */, const int64_t* ids, int64_t n,
                           const float* radius /* host n */, int32_t mode, int32_t negate, vs_sel** out);
#define VS_SEL_AND 0
#define VS_SEL_OR 1
#define VS_SEL_ANDNOT 2
#define VS_SEL_NOT 3
int vs_sel_combine(vs_index* index, const vs_sel* a, const vs_sel* b /* NULL for VS_SEL_NOT */, int32_t op,
                   vs_sel** out);
int vs_sel_bitmap(const vs_sel* sel, uint8_t* out /* host */, int64_t nbytes);
int vs_set_scoresel_staging_bytes(int64_t bytes); /* >= 1 */
/* last vs_sel_from_range / _rows on the handle, up to cap (5): {allowed rows m, members, tier taken (0: nothing
 * was scored, VS_RANGE_SCAN, VS_RANGE_SCREEN), queries re-answered by the scan, query blocks} */
int vs_scoresel_last_stats(vs_index* index, int64_t* out, int cap);
/* measurement hook (scripts/scoresel_timing.py): the last call on the handle, up to cap (3): ms of
 * HIP-event time {screen + refine, scan (+ fold), finish (mask, count, compact)} */
int vs_scoresel_last_times(vs_index* index, double* out, int cap);

/* ==== multi-device flat index (one process, several GPUs; SURVEY.md §8 b/e) =================
 * The reference holds ONE index in ONE process (main.py:59-68 -> utils/vector_store.py:72-81); this
 * handle keeps that contract over G devices.  Rows are dealt in chunks of 2^16 consecutive ids
 * (chunk j on dev_ids[j mod G]), so ids stay insertion order 0..ntotal-1 under incremental and bulk
 * adds.  vs_multi_search runs every shard's exact search concurrently (one host worker + stream per
 * device), maps local ids to global ids on each device, copies the per-shard (fp64 score, id) lists
 * to dev_ids[0] over xGMI peer copies and merges them there (vs_merge_shards_device's kernel):
 * results equal a single index over all rows.  Devices may repeat (several shards on one GPU).
 * Calls on one handle are serialised. */
typedef struct vs_multi vs_multi;

int vs_multi_create(int d, int metric, int dtype, int n_dev, const int* dev_ids, vs_multi** out);
void vs_multi_destroy(vs_multi* m);
int vs_multi_add(vs_multi* m, const float* x, int64_t n);                           /* host rows */
int vs_multi_add_from_file(vs_multi* m, const char* path, int64_t byte_offset, int64_t n);
int vs_multi_write_rows_to_file(vs_multi* m, const char* path, int64_t byte_offset, int64_t i0, int64_t n);
int vs_multi_search(vs_multi* m, const float* q, int64_t nq, int32_t k, float* D, int64_t* I);
/* vs_search_sel over the devices (SearchParameters.sel on the one index the reference would hold):
 * bitmap covers the global ids [0, ntotal) in IDSelectorBitmap's layout.  Rows are dealt in chunks of
 * 2^16 ids = 8192 bitmap bytes, so each shard's local bitmap is a gather of 8 KiB pieces of the
 * global one; a per-shard selector is built per call, the shards' filtered searches run as
 * vs_multi_search runs the unfiltered ones, and the same merge joins them. */
int vs_multi_search_sel(vs_multi* m, const uint8_t* bitmap, int64_t nbytes, const float* q, int64_t nq,
                        int32_t k, float* D, int64_t* I);
/* vs_range_search over the devices: bitmap (NULL = no filter) as in vs_multi_search_sel; every
 * shard's range search runs on its own worker and stream, local ids become global ids and each
 * query's shard segments are merged on the host under the same order.  Equals one index over all rows. */
int vs_multi_range_search(vs_multi* m, const uint8_t* bitmap, int64_t nbytes, const float* q, int64_t nq,
                          const float* radius, int64_t max_total, vs_range_result** out);
int vs_multi_reconstruct_n(vs_multi* m, int64_t i0, int64_t n, float* out);
int vs_multi_reset(vs_multi* m);
int vs_multi_set_screen(vs_multi* m, int screen);
int64_t vs_multi_ntotal(const vs_multi* m);
int vs_multi_ndev(const vs_multi* m);
int64_t vs_multi_shard_rows(const vs_multi* m, int shard);

/* ==== IVF-Flat (BASELINE cfg5) ===========================================
 * Not a reference call site: the reference's VectorStore offers flat and HNSW only
 * (utils/vector_store.py:51-53, 72-81).  This is the faiss IndexIVFFlat surface (faiss-cpu,
 * requirements.txt:5): IndexIVFFlat(quantizer, d, nlist, metric) -> vs_ivf_create,
 * .train -> vs_ivf_set_centroids (k-means runs in the Python layer over vs_ivf_assign, or on the
 * device over a flat index's rows: vs_kmeans),
 * .add -> vs_ivf_add, .search with .nprobe -> vs_ivf_search, .reconstruct -> vs_ivf_reconstruct.
 * Semantics (made exact, oracle/ivf_oracle.py): rows go to their exact best centroid (ties ->
 * lower list id) by its stored (dtype-rounded) values; a query probes its exact top-nprobe centroids and gets the exact top-k of the
 * rows of those lists (canonical fp64 score, ties -> lower id; -1 / worst-score padding).
 * Ids are insertion order 0..ntotal-1, as for the flat index.  Searches on one handle are
 * serialised; add/reset take an exclusive lock. */
typedef struct vs_ivf vs_ivf;

int vs_ivf_create(int d, int nlist, int metric, int dtype, int device, vs_ivf** out);
void vs_ivf_destroy(vs_ivf* ivf);
int vs_ivf_set_centroids(vs_ivf* ivf, const float* c);        /* host nlist x d; only while empty */
int vs_ivf_get_centroids(vs_ivf* ivf, float* out);            /* host nlist x d, values as stored */
int vs_ivf_is_trained(const vs_ivf* ivf);
int vs_ivf_assign(vs_ivf* ivf, const float* x, int64_t n, int64_t* lists); /* host; by the rows' dtype-rounded values */
int vs_ivf_add(vs_ivf* ivf, const float* x, int64_t n);       /* host fp32 n x d */
int vs_ivf_add_device(vs_ivf* ivf, const float* x_dev, int64_t n, void* stream); /* device fp32 n x d */
int vs_ivf_add_synthetic(vs_ivf* ivf, uint64_t seed, int64_t global_row0, int64_t n, int normalize);
/* size the HBM page pool for n more rows at once (chunked adds otherwise grow it by device copy,
 * which needs the old and the new pool side by side) */
int vs_ivf_reserve(vs_ivf* ivf, int64_t n);
int vs_ivf_search(vs_ivf* ivf, const float* q, int64_t nq, int32_t k, int32_t nprobe, float* D, int64_t* I);
/* device q/D/I/S64 (D, S64 may be NULL); host-synchronising (the probe -> work-item step). */
int vs_ivf_search_device(vs_ivf* ivf, const float* q_dev, int64_t nq, int32_t k, int32_t nprobe, float* D_dev,
                         int64_t* I_dev, double* S64_dev, void* stream);
int vs_ivf_reconstruct(vs_ivf* ivf, int64_t id, float* out);
int vs_ivf_list_sizes(vs_ivf* ivf, int64_t* out);             /* nlist entries */
int vs_ivf_reset(vs_ivf* ivf);                                /* drop rows, keep centroids */
int64_t vs_ivf_ntotal(const vs_ivf* ivf);
int vs_ivf_nlist(const vs_ivf* ivf);
/* bench: HIP events around the list-scan kernels of each search (same contract as vs_timing_fetch);
 * bytes_scanned (may be NULL) receives the algorithmic bytes those scans read, per search. */
int vs_ivf_set_timing(vs_ivf* ivf, int enable);
int vs_ivf_timing_fetch(vs_ivf* ivf, float* ms, double* bytes_scanned, int cap);
/* List-scan kernels (results are identical either way): VS_IVF_SCAN_AUTO (default) scans a list
 * probed by many queries with the MFMA screen over its pages (bf16/f16, once per 256 queries) when
 * a cost model says it beats re-reading it per 8 queries with the GEMV scan; _GEMV never does;
 * _MFMA does for every list probed by > 1 query (tests).  vs_ivf_last_search_stats reports the
 * first pass of the last search: its MFMA list scans, the queries its certificate rejected
 * (re-searched together, deeper) and the page bytes the MFMA and the GEMV scans read, re-reads
 * included (bytes_read[0], [1]); any pointer may be NULL. */
#define VS_IVF_SCAN_AUTO 0
#define VS_IVF_SCAN_GEMV 1
#define VS_IVF_SCAN_MFMA 2
int vs_ivf_set_scan(vs_ivf* ivf, int mode);
/* Query tiles of the MFMA list scans' first pass (results are identical either way):
 * VS_IVF_QTILE_SPLIT (default) packs (hi, lo) parts of each query (128 queries a tile, two MFMA
 * columns per query); VS_IVF_QTILE_PLAIN packs each query once, rounded to the list dtype (256
 * queries a tile; lists probed by <= 64 queries take the narrow 64-column form), its ~2^8 x wider
 * rounding margin taken by the certificate, so more queries may need a re-search.  Re-search
 * rounds always pack split tiles; plain tiles need the direct form (padded dim a multiple of 128),
 * otherwise split tiles are used. */
#define VS_IVF_QTILE_PLAIN 0
#define VS_IVF_QTILE_SPLIT 1
int vs_ivf_set_query_tiles(vs_ivf* ivf, int mode);
int vs_ivf_last_search_stats(const vs_ivf* ivf, int* mfma_lists, int* uncertified, double* bytes_read);

/* ==== HNSW graph search ===================================================
 * Replaces the search of faiss.IndexHNSWFlat, which the reference builds for
 * index_type="hnsw" (utils/vector_store.py:73-78: IndexHNSWFlat(d, M, metric), hnsw.efSearch) and
 * searches at utils/vector_store.py:191.  A vs_hnsw is a graph in faiss's HNSW layout (the arrays
 * of an IHNf file: node levels, per-node offsets into the neighbour array, cumulative neighbour
 * counts per level, entry point, max level) over the rows of a flat vs_index (graph node i = row
 * i); the graph is copied to the index's device and validated (ids in range, neighbours present
 * on their level, offsets matching the levels); a later duplicate in a neighbour list is dropped,
 * which changes no search.  vs_hnsw_search runs faiss HNSW::search (greedy descent on the upper
 * levels, then efSearch-bounded best-first search on level 0; oracle/hnsw_oracle.py) on the GPU,
 * one workgroup per query, with the flat path's exact canonical scores as distances: D = scores
 * (IP) / squared distances (L2) best first, I = row ids, -1 padded.  The graph covers the first
 * n rows of the index: rows added behind it are not reachable (the caller searches them exactly
 * and merges); an index holding fewer than n rows is VS_ERR_ARG; max(ef_search, k) <= 2048.  A graph
 * is stale once the index was reset or rows were removed from it (vs_reset, vs_remove_ids: node i is
 * no longer row i): vs_hnsw_search and vs_hnsw_patch on it are VS_ERR_ARG. */
typedef struct vs_hnsw vs_hnsw;

int vs_hnsw_create(vs_index* index, int64_t n, const int32_t* levels, const uint64_t* offsets,
                   const int32_t* neighbors, const int32_t* cum_nneighbor_per_level, int32_t n_cum,
                   int32_t entry_point, int32_t max_level, vs_hnsw** out);
void vs_hnsw_destroy(vs_hnsw* graph);
int vs_hnsw_search(vs_hnsw* graph, const float* q, int64_t nq, int32_t k, int32_t ef_search, float* D,
                   int64_t* I);
int64_t vs_hnsw_ntotal(const vs_hnsw* graph);
/* Rewrite m neighbour slots (positions into the create call's neighbour array) and set the entry
 * point / top level: the batched insertion of faiss IndexHNSWFlat.add (utils/vector_store.py:164)
 * keeps ONE device graph laid out for the final node count -- nodes not inserted yet have empty
 * lists and no links to them, so they are unreachable -- and patches in each batch's new lists
 * and reverse links (photo_search_engine_amd/hnsw.py insert_rows).  Slots and ids are validated
 * as in vs_hnsw_create, and a patch must rewrite whole (node, level) lists -- every slot of each list
 * it touches -- each as distinct ids followed by -1s (VS_ERR_ARG otherwise, the graph unchanged). */
int vs_hnsw_patch(vs_hnsw* graph, int64_t m, const uint64_t* pos, const int32_t* val, int32_t entry_point,
                  int32_t max_level);

/* HNSW graph build: faiss HNSW::shrink_neighbor_list (the neighbour-selection heuristic
 * IndexHNSWFlat.add applies to a new node's candidates and to a full list receiving a reverse link,
 * utils/vector_store.py:164) for m nodes at once on the GPU.  nodes[i] = row id of node i;
 * cand[i * C ..] = its distinct candidate row ids, -1 padded at the end; with fewer than W
 * candidates all are kept (faiss returns early below max_size), else candidates are taken in
 * ascending (distance, id) order and one is kept unless an already kept neighbour is strictly closer
 * to it than the node is, up to W.  Distances are the flat path's canonical fp64 scores (IP: -score).
 * out[i * W ..] = kept ids best first, -1 padded.  C <= 2048, W <= 1024; ids are validated. */
int vs_hnsw_prune(vs_index* index, int64_t m, const int64_t* nodes, const int32_t* cand, int32_t C, int32_t W,
                  int32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* VS_H_ */
