// vs_internal.h -- shared constants, HBM layout and kernel launchers of libvs (gfx950 only).
//
// HBM layout of a corpus shard ("row tiles"):
//   rows are grouped in tiles of TR = 256; a chunk is CE = CHB / es elements (32 fp32, 64 bf16 /
//   f16), one 128 B line per row; d is padded to dpad = roundup(d, CE) (>= 64);
//   inside a tile the matrix is stored chunk-major: [chunk c = i / CE][row r in tile][CE elements]
//   so element (r, i) of a tile lives at  c*(TR*CHB) + (r % TR)*CHB + (i % CE)*es.
// A row's piece of a chunk fills one 128 B line, so the exact-rescoring gather of a candidate row
// fetches only that row's bytes.  One MFMA K-step (256 rows x 32 bf16 elements) reads the
// 64 B half of every row's line (the next K-step the other half, from L2); every global load is
// a 16 B/lane piece of a 64 B run.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <stdexcept>
#include <string>

#include "../../include/vs.h"

namespace vs {

constexpr int TR = 256;        // rows per tile
constexpr int CH = 32;         // elements per MFMA K-step (bf16 / f16: half a chunk)
constexpr int CHB = 128;       // bytes of a row's piece of one chunk: one 128 B line
constexpr int DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2;
constexpr int DT_I8 = 3;        // internal: the int8 screen copy (per-row scale, exact int32 MFMA)
constexpr int METRIC_IP = 0, METRIC_L2 = 1;

constexpr int MFMA_QB = 256;   // queries per MFMA screen launch
constexpr int MF_WG_THREADS = 512;  // MFMA screen workgroup (8 waves)
constexpr int MFMA_CAP = 768;  // candidate slots per (workgroup, query) in the MFMA screen
constexpr int MFMA_KP_MAX = 512;  // per-(workgroup, query) screening depth of the MFMA screen (= MFMA_CAP - TR:
                                  // a compacted buffer plus one tile fits); deeper searches keep 512 per
                                  // workgroup and certify against the workgroups' drop bounds
static_assert(MFMA_KP_MAX + TR <= MFMA_CAP, "MFMA screen: compaction invariant cnt <= cap - TR");
constexpr int GEMV_NQ_MAX = 8; // queries per GEMV screen launch
constexpr int GEMV_SPLIT = 4;   // row blocks per tile of the GEMV screen's small-corpus work items
constexpr int KP_MAX = 4096;   // largest screening depth (k <= 3276; k_refine sorts 4096 keys in LDS)
// the largest k of an exact search: its screen lists k + k / 4 rows (screen_depth), KP_MAX at the most
constexpr int K_MAX = KP_MAX * 4 / 5;
constexpr int SELECT_E = 16;   // keys per thread in block selection (256 threads -> 4096 keys)

inline int es_of(int dt) { return dt == DT_F32 ? 4 : 2; }
// padded dimension of the tiled layout: whole chunks, >= 2 MFMA K-steps per tile (the screen's
// deferred compaction check runs on the K-step after a tile's epilogue)
inline int pad_dim(int d, int dt) {
    const int ce = CHB / es_of(dt);
    return (int)std::max<int64_t>(((int64_t)d + ce - 1) / ce * ce, 2 * CH);
}
inline int64_t tile_bytes(int dpad, int dt) { return (int64_t)TR * dpad * es_of(dt); }
inline int64_t round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }

// the query as fp64 in LDS: (d + 7) / 8 groups of 8 elements
__host__ __device__ inline size_t query_lds_bytes(int d) { return (size_t)((d + 7) >> 3) * 64; }

// the least floor * 2^i that is >= n (floor: a power of two)
inline int64_t pow2_at_least(int64_t n, int64_t floor) {
    int64_t p = floor;
    while (p < n) p <<= 1;
    return p;
}

constexpr int RFW_CAP = 8192;  // k_refine_wide: rows scored per query (fp64 score + id in LDS)
// k_refine_wide's phase A takes between KA and this many keys (the two-phase state holds as many):
// up to 1.5 KA, within KA's power of two (the phase-A sort's size stays what KA alone gives)
__host__ __device__ inline int rfw_ka_hi(int KA) {
    int p2 = 1;
    while (p2 < KA) p2 <<= 1;
    const int hi = KA + KA / 2 < p2 ? KA + KA / 2 : p2;
    return hi > KA ? hi : KA;
}

// screening depth: k plus a margin that certifies exactness for all but pathological inputs
inline int screen_depth(int k) {
    int kp = k + std::max(16, k / 4);
    kp = (int)round_up(kp, 16);
    return std::min(kp, KP_MAX);
}

// fp32 accumulation error factor of a d-term dot product (chains of <= d + 64 roundings)
inline float gamma_of(int d) {
    const double u = 5.9604644775390625e-08;  // 2^-24
    const double n = (double)d + 64.0;
    return (float)(n * u / (1.0 - n * u));
}

// ---- errors: C++ exceptions inside the library, int codes + vs_last_error() at the ABI --------
struct VsError : std::runtime_error {
    int code;
    VsError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
void set_last_error(const std::string& msg);  // thread-local message read by vs_last_error()

#define HIP_CHECK(expr)                                                                                    \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess)                                                                              \
            throw ::vs::VsError(_e == hipErrorOutOfMemory ? VS_ERR_OOM : VS_ERR_DEVICE,                    \
                                std::string(#expr) + ": " + hipGetErrorString(_e));                        \
    } while (0)

template <typename F>
int guarded(F&& f) {
    try {
        f();
        return VS_OK;
    } catch (const VsError& e) {
        set_last_error(e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return VS_ERR_INTERNAL;
    } catch (...) {
        set_last_error("unknown error");
        return VS_ERR_INTERNAL;
    }
}

// live bytes of every DevBuf in the process (vs_device_bytes_live)
inline std::atomic<int64_t> g_dev_bytes_live{0};

// device buffer that only grows; owns its allocation (move-only), freed with its device current
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(bytes, o.bytes);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void ensure(size_t want) {
        if (want <= bytes) return;
        release();
        HIP_CHECK(hipMalloc(&p, want));
        bytes = want;
        g_dev_bytes_live.fetch_add((int64_t)want, std::memory_order_relaxed);
    }
    template <typename T>
    T* as() const { return (T*)p; }
    void release() {
        if (p) {
            (void)hipFree(p);
            g_dev_bytes_live.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
        }
        p = nullptr;
        bytes = 0;
    }
};

// pinned host staging (grow-only, move-only): pageable hipMemcpyAsync is a staged, blocking copy
struct HostBuf {
    void* p = nullptr;
    size_t bytes = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    HostBuf(HostBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
        o.p = nullptr;
        o.bytes = 0;
    }
    HostBuf& operator=(HostBuf&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(bytes, o.bytes);
        }
        return *this;
    }
    ~HostBuf() { release(); }
    void ensure(size_t want) {
        if (want <= bytes) return;
        release();
        HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
        bytes = want;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// an event that destroys itself (move-only); empty until create()
struct DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    explicit DevEvent(unsigned flags) { create(flags); }
    DevEvent(const DevEvent&) = delete;
    DevEvent& operator=(const DevEvent&) = delete;
    DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
    DevEvent& operator=(DevEvent&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(e, o.e);
        }
        return *this;
    }
    ~DevEvent() { release(); }
    void create(unsigned flags = hipEventDefault) {
        if (!e) HIP_CHECK(hipEventCreateWithFlags(&e, flags));
    }
    void release() {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    operator hipEvent_t() const { return e; }
};

// two pinned host chunks + their "chunk consumed" events: double buffering of host <-> HBM copies
struct PinnedPair {
    HostBuf chunk[2];
    DevEvent done[2];
    float* host(int b) const { return (float*)chunk[b].p; }
    void ensure(size_t want) {
        done[0].create(hipEventDisableTiming);
        done[1].create(hipEventDisableTiming);
        if (want <= chunk[1].bytes) return;
        release_host();
        chunk[0].ensure(want);
        chunk[1].ensure(want);
    }
    void release_host() {
        for (HostBuf& h : chunk) h.release();
    }
    void release() {
        release_host();
        for (DevEvent& e : done) e.release();
    }
};

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) HIP_CHECK(hipSetDevice(dev));
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

// candidate key: (orderable score << 32) | (0xFFFFFFFF - local id); larger key = better,
// equal scores -> lower id first; key 0 = empty slot.
typedef unsigned long long u64;

struct ScreenArgs {
    const uint8_t* corpus;   // tiled shard
    int64_t n_valid;         // rows in the shard
    int tiles;               // ceil(n_valid / TR)
    int dpad, d;
    int metric;
    const float* sqn;        // per-row ||x||^2 (fp32) for L2 screening
    int Kp;                  // screening depth per (workgroup, query)
    int cap;                 // candidate buffer slots per (workgroup, query)
    u64* cand;               // [G][QB][cap]
    u64* part;               // [G][QB][Kp]
    int G;                   // workgroups
    int tile_stride;         // > 0: workgroup b screens only tile b*tile_stride (threshold seeding)
    const u64* thr0;         // [QB] initial per-query key threshold (keys > thr0 kept), or null
    float* seedmax;          // seed pass only: [QB][G*16] maxima of disjoint 16-row groups per query
    u64* glist;              // MFMA path output: per-query compact survivor list [QB][lcap] ...
    int* gcnt;               // ... with its length per query (zeroed by k_pack_qtile)
    int lcap;                // = G * Kp
    int* next_tile;          // GEMV: tile work-queue counter (zeroed before the launch); null = static ranges
    float* seed_acc;         // MFMA: [G][512 lanes][128] raw accumulators of each workgroup's seed tile (the
                             // first tile of its range): written by the seed pass, reused by the main pass
    const uint32_t* rsb;     // int8 screen, per row: bf16 scale s_x (x_hat = s_x * codes) in the low half,
                             // bf16 ||x - x_hat||_2 rounded up in the high half
    const float2* qfac;      // int8 screen: per query (t_q, ||q||), codes q_hat = t_q * int8
    const float* qinfo;      // int8 GEMV: per query [2q] = ||q|| rounded up (k_pack_qf32)
    u64* drop;               // MFMA: per query, max over workgroups of their compaction threshold
                             // (rows below it were dropped; zeroed by the query pack), or null
    const int* gate;         // device fallback round: the launch does nothing while *gate == 0 (no
                             // query of the block failed its certificate), or null = always run
    const int* tile_map;     // mapped screen (IVF list scan): page of logical tile t; keys carry
                             // storage slots page * TR + row, n_valid counts the list's rows
    const int* qmap;         // mapped screen: glist / gcnt row of a query (the workgroup's slice below)
    const int* skip;         // device fallback round: queries with skip[q] != 0 (certified by the first
                             // pass) are not screened (threshold +inf: no candidates), or null
    const int* wg_desc;      // mapped screen: per workgroup MAP_DESC ints {tile_map offset of its
                             // first tile, tiles, logical index of the first tile in its list
                             // segment, rows of that segment, query tile index, qmap offset, queries}
    int gemv_split;          // GEMV screen: 1 (or 0) = work items of whole tiles, GEMV_SPLIT = of
                             // 256 / GEMV_SPLIT rows (small corpora: more CUs)
    const float* gT;         // int8 group residuals: [group][QB] <mu_g, q> added to every key of the
                             // group's rows (the seed pass and k_screen_i8d_res), or null
    unsigned long long* stamps;  // diagnostic probe forms only (vs_k1probe.hip): per workgroup
                                 // {s_memtime, s_memrealtime} around the loop; null in the product
};
constexpr int MAP_DESC = 8;
constexpr int MFMA_MAP_TILES = 256;  // mapped screen: logical tiles per workgroup (its LDS page table)
int gemv_blocks_per_cu(int dt, int nqpad, int dpad);  // resident k_screen_gemv blocks per CU (occupancy API)

// ---- launchers (vs_kernels.hip) -------------------------------------------------------------
hipError_t launch_pack_rows(int dt, const float* src, int64_t n, int d, int dpad, uint8_t* data, int64_t lrow0,
                            float* sqn, unsigned* maxsq, hipStream_t st);
hipError_t launch_synth_rows(int dt, uint64_t seed, int64_t grow0, int64_t n, int d, int dpad, uint8_t* data,
                             int64_t lrow0, int normalize, float* sqn, unsigned* maxsq, hipStream_t st);
hipError_t launch_synth_f32(int dt, uint64_t seed, int64_t grow0, int64_t n, int d, int normalize, float* out,
                            hipStream_t st);
hipError_t launch_unpack_rows(int dt, const uint8_t* data, int64_t lrow0, int64_t n, int d, int dpad, float* out,
                              hipStream_t st);
hipError_t launch_gather_rows(int dt, const uint8_t* data, const int64_t* ids, int64_t n, int d, int dpad,
                              float* out, hipStream_t st);

// queries: MFMA tile (dtype, [nks][256][32]) or fp32 padded [NQ][dpad]; qinfo[q*2] = ||q_hat||,
// qinfo[q*2+1] = ||q_hat - q|| (upper bounds, fp32)
// fails (optional): zeroed -- the query block's certificate-failure count (RefineArgs::fails);
// gate (optional): as ScreenArgs::gate
// qidx (optional): tile row r packs query qidx[r] of q; qinfo is then indexed by qidx and max-combined
hipError_t launch_pack_qtile(int dt, const float* q, int nqb, int d, int dpad, uint8_t* qt, float* qinfo, int* gcnt,
                             u64* drop, hipStream_t st, int* fails = nullptr, const int* gate = nullptr,
                             const int* qidx = nullptr,
                             int* gcnt2 = nullptr, u64* drop2 = nullptr);
hipError_t launch_pack_qf32(const float* q, int nqb, int nqpad, int d, int dpad, float* qp, float* qinfo,
                            hipStream_t st, int* ctr = nullptr,  // ctr: zeroed (a screen's tile queue)
                            int* fails = nullptr, u64* drop = nullptr);  // drop: zeroed [nqpad]

hipError_t launch_screen_mfma(int dt, const ScreenArgs& a, const uint8_t* qt, int nqb, hipStream_t st);
// the direct K1 screens' schedule: 0 = barrier at the head of every K-step, 1 = mid-step barrier
void set_k1_schedule(int s);
int k1_schedule();
// diagnostic forms of the direct screen (vs_k1probe.hip): variant = VS_K1P_* (include/vs.h)
hipError_t launch_k1_probe(int variant, int dt, const ScreenArgs& a, const uint8_t* qt, int nqb, hipStream_t st);
// the int8 main pass runs the direct form (k_screen_i8d) for this int8 row stride (K-steps per tile
// a multiple of 4); it takes no seed-tile accumulators (ScreenArgs::seed_acc must be null)
bool i8_direct_ok(int dpad8);
// the same for bf16 / f16 rows (k_screen_d16: K-steps of 32 elements per tile a multiple of 4)
bool d16_direct_ok(int dpad);
// the same screen over pages of a page pool (IVF lists; bf16 / f16, unseeded, a.Kp <= MFMA_KP_MAX):
// a.G workgroups, each with its own descriptor (a.wg_desc): <= MFMA_MAP_TILES pages of one list
// (a.tile_map), one query tile of <= 128 split queries or <= 256 plain ones (qt + index * MFMA_QB *
// dpad * 2, made by launch_pack_qtile_split); survivors appended to glist rows a.qmap[...].
// Descriptors are validated on the host (check_map_desc) before the launch.  plain: the direct
// form only (d16_direct_ok).
hipError_t launch_screen_mfma_mapped(int dt, const ScreenArgs& a, const uint8_t* qt, bool plain, hipStream_t st);
// host check of one descriptor against the launch (tile map length, query tiles, qmap length)
bool check_map_desc(const int* desc, int64_t tmap_len, int n_qtiles, int64_t qmap_len, bool plain);
// every query tile of the launch at once: tile y packs the sinfo[2y + 1] (1..128 split, 1..256
// plain) queries qidx[sinfo[2y] ..] of q (host-checked by the caller)
hipError_t launch_pack_qtile_split(int dt, const float* q, const int* qidx, const int* sinfo, int ntiles, int d,
                                   int dpad, uint8_t* qt, float* qinfo, bool plain, hipStream_t st);
hipError_t launch_screen_gemv(int dt, const ScreenArgs& a, const float* qp, int nqb, int nqpad, hipStream_t st);

// one merge stage: in[(s*qstride + q)*Kp + j], s < nseg  ->  out[(b*nq + q)*Kp + j]
hipError_t launch_merge(const u64* in, int nseg, int qstride, int nq, int Kp, u64* out, int* nseg_out,
                        hipStream_t st);

constexpr int kRefineOneWaveKeys = 2048;  // = 64 * RF_WE: lists one wave of k_refine selects from
constexpr int kRefineRegKeys = 16384;     // = RF_THREADS * RF_E: lists k_refine selects from in registers
struct RefineArgs {
    const u64* cand;       // [nq][lcap] candidate keys: the first cand_n[q] (or, if cand_n is null,
    const int* cand_n;     //  all lcap, zero = empty) of each row; the refine keeps the best Kp
    int lcap;
    int Kp;
    const float* q;        // [nq][d] fp32 (original queries)
    int d, dpad, dt, metric;
    const uint8_t* corpus;
    const float* qinfo;    // [nq][2]
    float xmax;            // upper bound on ||x|| over the shard
    float gamma;           // fp32 accumulation error factor
    int k;
    int64_t n_valid;
    int64_t id_offset;
    float* D;              // [nq][k] (may be null)
    int64_t* I;            // [nq][k]
    double* S64;           // [nq][k] (may be null)
    int* cert;             // [nq] 1 = certified exact (may be null)
    unsigned* uncert;      // device counter (may be null)
    int optimistic;        // screened with an optimistic seed: fewer than Kp candidates = uncertified
    const float* qeps;     // int8 screen (k_refine_wide): per query, true score <= key_score + qeps
                           //  (negative where the query's int8 error earns a credit, k_pack_qtile_i8)
    unsigned long long* rows;  // k_refine_wide: device count of the rows it scores (or null)
    const u64* drop;       // MFMA: per query, the workgroups' largest compaction threshold (or null)
    const u64* thr0;       // the screen's starting threshold per query (or null = none)
    const unsigned* i8max; // int8 GEMV screen: (max ||x_hat||, max beta) fp32 bits -> the certificate margin
    const uint32_t* idmap; // IVF: user id of every storage slot (keys carry slots); null = identity
    int* fails;            // first pass: count of the block's uncertified queries (the fallback's gate)
    int redo;              // device fallback round: only queries with cert[q] == 0 are refined (and
    const int* gate;       //  their outputs rewritten), nothing at all while *gate == 0
    int nsplit;            // k_refine, few queries with deep lists: > 1 workgroups per query each score
    double* gsc;           //  a slice of the kept rows into gsc / gids ([nq][KP2]); the last one to
    uint32_t* gids;        //  finish (gdone[q], zero between launches) sorts and certifies.  0/1 =
    unsigned* gdone;       //  one workgroup per query.
    // k_refine_wide in two launches around an exchange (the sharded step, vs_search_device_phase_a
    // / _phase_b): phase 1 scores the best KA keys and stops -- the top-k of them go to (D, I, S64)
    // for the exchange, the scored rows to pa_* -- and phase 2 resumes from pa_* with the floor
    // tfloor[q * tfloor_k + tfloor_k - 1] (a lower bound of the global k-th best score, metric
    // domain: IP score / L2 distance) raising T'.  0 = one launch (both phases).
    int phase;
    double* pa_sc;         // [nq][pa_cap] phase-1 scored rows (sorted, worst-padded), their ids,
    uint32_t* pa_ids;      //  count and phase-A key threshold
    int* pa_n;
    u64* pa_tA;
    int pa_cap;
    const double* tfloor;
    int tfloor_k;
    int ostride;           // I / S64 element stride (0/1 = separate arrays; 2 = interleaved (score bits, id))
};
// k_refine's kept-row capacity: a power of two >= 1.5 Kp (<= KP_MAX, >= Kp): its selection stops at
// any count of the best keys in [Kp, refine_kp2(Kp)], which ends the bisection early
inline int refine_kp2(int Kp) {
    const int want = std::max(Kp, std::min(KP_MAX, Kp + Kp / 2));
    return (int)pow2_at_least(want, 1);
}
// workgroups per query of k_refine for a Kp-deep refine of nq queries (1 = no split)
int refine_split(int nq, int Kp, int dt, int num_cu);
hipError_t launch_refine(const RefineArgs& a, int nq, hipStream_t st);
// exact refine behind the int8 screen: adaptive two-phase depth (KA keys first), IP only
hipError_t launch_refine_wide(const RefineArgs& a, int nq, int KA, hipStream_t st);
// exact full scan of a shard for the queries no bounded screen could certify (vs_fullscan.hip):
// every row scored canonically, streamed through a running top-k (any number of ties)
struct FullScanArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;
    const float* q;         // [nq][d] fp32 queries of the block
    int nq, k;
    int* cert;              // [nq]: queries with cert[q] == 0 are scanned (and set to 1)
    const int* gate;        // nothing at all while *gate == 0 (the fallback round's failure count), or null
    int64_t id_offset;
    float* D;               // [nq][k] (may be null)
    int64_t* I;             // [nq][k]
    double* S64;            // [nq][k] (may be null)
    int ostride;            // I / S64 element stride, as RefineArgs::ostride
    double* gsc;            // [nq][G][k] per-workgroup lists (full_scan_scratch_bytes)
    uint32_t* gid;
    unsigned* gdone;        // [nq] per-query completion counters, zero between launches
    unsigned* count;        // queries scanned (device counter), or null
    int G;                  // workgroups (row ranges)
    int all_queries;        // 1: scan every query of the block (cert is only written), no memset first
};
constexpr int FS_THREADS = 512;  // threads of a scan workgroup
constexpr int FS_B = 512;        // candidate batch merged into a workgroup's list at once; also the most workgroups (G)
size_t full_scan_scratch_bytes(int nq, int G, int k);
void set_lds_attr(const void* fn, int bytes);  // max dynamic LDS of a kernel, set once per device
hipError_t launch_full_scan(const FullScanArgs& a, hipStream_t st);

// ---- id selectors (vs_selscan.hip) -------------------------------------------------------------
// device bitmap (64-bit words, faiss IDSelectorBitmap's bit order) -> ascending ids of [0, n_sel) and
// their count; wgsum: sel_compact_groups(n_sel) words of scratch; ids holds cap entries (the host's
// count of the same bitmap under the same masking)
int64_t sel_compact_groups(int64_t n_sel);
hipError_t launch_sel_compact(const uint64_t* bits, int64_t n_sel, unsigned* wgsum, uint32_t* ids, int64_t cap,
                              unsigned long long* count, hipStream_t st);
// the full scan's streaming exact top-k over the m listed rows (ids ascending, each < a.n_valid);
// a.G workgroups split the list, qy (1..a.nq) query slices deal the block's queries (grid a.G x qy);
// a.cert / a.all_queries as in launch_full_scan (m < a.k: padded)
hipError_t launch_sel_scan(const FullScanArgs& a, const uint32_t* ids, int64_t m, int qy, hipStream_t st);
// the allowed entries of exact unfiltered lists [nq][kp] (best first, -1 padded), the first k each
struct SelTakeArgs {
    const uint64_t* bits;   // the selector's bitmap
    int64_t n_sel;          // ids at or past it are not selected
    const int64_t* I_in;    // [nq][kp]
    const float* D_in;      // [nq][kp] (with D)
    const double* S_in;     // [nq][kp] (with S64)
    int kp, k, metric;
    float* D;               // [nq][k] (may be null)
    int64_t* I;             // [nq][k]
    double* S64;            // [nq][k] (may be null)
    const int* cert_in;     // [nq] the unfiltered search's certificates
    int* found;             // [nq] allowed entries found, capped at k
    int* cert_out;          // [nq] 1 = the filtered prefix is proven (k found, or the list is exhaustive)
    int exhaustive;         // the unfiltered lists hold every row of the index
};
hipError_t launch_sel_take(const SelTakeArgs& a, int nq, hipStream_t st);

// ---- row removal (vs_remove.hip) ---------------------------------------------------
// bits[w] = ~bits[w] for the nwords words of a device bitmap (removed rows -> kept rows; the
// compaction masks the bits at or past the row count)
hipError_t launch_remove_complement(uint64_t* bits, int64_t nwords, hipStream_t st);
// destination tiles [t0, t0 + nt) of the compacted shard, written into the bounce buffer as final
// tiles: new row j = old row src[j] (ascending, src[j] >= j, j < n_new; the rows of the last tile
// at or past n_new are zeroed).  A row is nchunks 128 B lines (tile_bytes = nchunks * TR * CHB);
// sqn_out [nt * TR] receives sqn[src[j]] alongside (0 past n_new).
hipError_t launch_remove_gather(const uint8_t* data, int64_t tile_bytes, int nchunks, const uint32_t* src,
                                int64_t n_new, int64_t t0, int64_t nt, uint8_t* stage, const float* sqn,
                                float* sqn_out, hipStream_t st);
// the bounce buffer over tiles [t0, t0 + nt) of the shard, and its sqn entries over theirs
hipError_t launch_remove_place(const uint8_t* stage, int64_t tile_bytes, int64_t t0, int64_t nt, uint8_t* data,
                               const float* sqn_stage, float* sqn, hipStream_t st);
// *maxsq = max(*maxsq, bits of max sqn[0, n)) (the caller zeroes it first)
hipError_t launch_remove_maxsq(const float* sqn, int64_t n, unsigned* maxsq, hipStream_t st);

// ---- range search (vs_range.hip) ---------------------------------------------------------------
// Every row whose fp32 score D = (float)S passes a per-query radius (D > r inner product, D < r L2),
// collected as (S, id) pairs in per-query regions of a pair buffer: query q appends at
// psc / pid[off[q] + pos], pos taken from cnt[q] by an atomic add; a pair is stored only while
// pos < cap[q], cnt[q] keeps counting past it (the host reruns the query with a region of that size).
constexpr int RS_SORT_MAX = 4096;  // longest segment k_range_emit sorts in LDS (sort_valid_best_first)
struct RangeArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;
    const float* q;         // [nq][d] fp32 queries of the block
    int nq;
    const float* radius;    // [nq]
    const int* go;          // [nq]: queries with go[q] == 0 are left alone, or null = every query
    double* psc;            // pair buffer: canonical fp64 scores (IP score / squared L2 distance) ...
    uint32_t* pid;          // ... and local row ids
    const int64_t* off;     // [nq] first slot of the query's region
    const int64_t* cap;     // [nq] slots of the region (0 = count only)
    unsigned long long* cnt;  // [nq] passing rows found (zeroed by the host before the launch)
    // queries taken from stored rows (vs_range_search_rows): self[q] = the row query q was gathered
    // from; VS_SELF_DROP rejects that row, VS_SELF_ABOVE every row with id <= self[q], before it is
    // counted.  row0 (ABOVE without a selector): no self id of the block is below it, so the scan
    // tier's sequence is [row0, n_valid).  A value-initialised struct (null, VS_SELF_KEEP, 0) is the
    // plain range search: it launches the kernels' instantiation that reads none of the three.
    const int64_t* self;
    int self_mode;
    int64_t row0;
};
// SCAN tier: G workgroups split the n_valid rows, or the m listed rows ids[0, m) (ascending, each <
// n_valid) when ids is given; qy (1..nq) query slices deal the block's queries (grid G x qy)
hipError_t launch_range_scan(const RangeArgs& a, int G, int qy, const uint32_t* ids, int64_t m, hipStream_t st);
// SCREEN tier, threshold: thr0[q] = a key below every key the native screen can give a row that
// passes radius[q] (0 = keep every row); qinfo / xmax / gamma as RefineArgs
hipError_t launch_range_thr(int metric, const float* radius, const float* qinfo, const float* q, int d, int nq,
                            float xmax, float gamma, u64* thr0, hipStream_t st);
// SCREEN tier, refine: the survivors glist[q][0, min(gcnt[q], lcap)) scored exactly and tested; ny
// workgroups per query share a list
hipError_t launch_range_refine(const RangeArgs& a, const u64* glist, const int* gcnt, int lcap, int ny,
                               hipStream_t st);
// one query's segment of the pair buffers -> its place in the block's outputs
struct RangeSeg {
    int64_t src;  // first slot in pair buffer `buf`
    int64_t n;    // pairs
    int64_t dst;  // first output slot
    int buf;      // 0 / 1
    int pad;
};
struct RangeEmitArgs {
    const double* psc[2];
    const uint32_t* pid[2];
    const RangeSeg* seg;  // [nq]
    int metric;
    int64_t id_offset;
    float* D;             // outputs: D = (float)S, I = id + id_offset, S
    int64_t* I;
    double* S;
};
// one workgroup per query: segments of at most RS_SORT_MAX pairs are written best first (S, then
// the lower id), longer ones as they are (the host sorts them)
hipError_t launch_range_emit(const RangeEmitArgs& a, int nq, hipStream_t st);

// ---- facet counts (vs_facet.hip) ------------------------------------------------------
// The range scan and the range refine with a histogram in place of the pair buffer (vs_range_scan.h):
// hist[q][bin] += 1 per member row that passes radius[q], bin = gid[row] for a grouped row, bins - 1 for
// an ungrouped one (gid null: bins == 1, everything in bin 0).
constexpr int FACET_LDS_BINS = VS_FACET_LDS_BINS;  // most bins of the LDS form (32 KiB of uint32)
struct FacetArgs {
    const int32_t* gid;        // [n_cov] group codes (vs_groups), or null
    int64_t n_cov;             // rows at or past it are no members
    int bins;                  // G + 1 (gid null: 1)
    unsigned long long* hist;  // [nq][bins] (zeroed by the host)
};
// as launch_range_scan / launch_range_refine; of RangeArgs only corpus, d, dpad, dt, metric, n_valid, q,
// nq, radius and go are read (self_mode must be VS_SELF_KEEP, row0 0).  lds: the LDS form, bins <=
// FACET_LDS_BINS.  The refine's form is always the global one.
hipError_t launch_facet_scan(const RangeArgs& a, const FacetArgs& f, bool lds, int G, int qy, const uint32_t* ids,
                             int64_t m, hipStream_t st);
hipError_t launch_facet_refine(const RangeArgs& a, const FacetArgs& f, const u64* glist, const int* gcnt, int lcap,
                               int ny, hipStream_t st);

// ---- score selectors (vs_scoresel.hip) ------------------------------------------------
// The range scan and the range refine with a bitmap in place of the pair buffer (vs_range_scan.h): a row
// that passes radius[q] sets bit (row & 63) of word bits[q * stride_words + (row >> 6)].  stride_words 0:
// the block's queries share one bitmap of ceil(n_valid / 64) words; otherwise each has its own, stride_words
// (>= that many) apart.  Bits are only ever set: the host zeroes what it wants zero.
struct BitsArgs {
    unsigned long long* bits;
    int64_t stride_words;
};
// as launch_range_scan / launch_range_refine; of RangeArgs only corpus, d, dpad, dt, metric, n_valid, q,
// nq, radius and go are read (self_mode must be VS_SELF_KEEP, row0 0)
hipError_t launch_bits_scan(const RangeArgs& a, const BitsArgs& b, int G, int qy, const uint32_t* ids, int64_t m,
                            hipStream_t st);
hipError_t launch_bits_refine(const RangeArgs& a, const BitsArgs& b, const u64* glist, const int* gcnt, int lcap, int ny,
                              hipStream_t st);
// acc[w] &= qbits[q * nwords + w] for every q < nqb, w < nwords
hipError_t launch_bits_fold(uint64_t* acc, const uint64_t* qbits, int nqb, int64_t nwords, hipStream_t st);
// out[w] = (negate ? ~acc[w] : acc[w]) & members[w] over the ceil(n_sel / 64) words of a bitmap over rows
// [0, n_sel), the bits at or past n_sel zero; members: a bitmap over rows [0, n_members), n_members <= n_sel,
// read as zero past its end (has_members false: every row); *total += the bits set in out
hipError_t launch_bits_finish(const uint64_t* acc, bool has_members, const uint64_t* members, int64_t n_members,
                              int negate, int64_t n_sel, uint64_t* out, unsigned long long* total, hipStream_t st);
// out = a op b (VS_SEL_AND / _OR / _ANDNOT; VS_SEL_NOT: ~a, b unused) over rows [0, n_sel); a covers rows
// [0, na), b rows [0, nb), each read as zero past its end; tail and *total as launch_bits_finish
hipError_t launch_bits_op(const uint64_t* a, int64_t na, const uint64_t* b, int64_t nb, int op, int64_t n_sel,
                          uint64_t* out, unsigned long long* total, hipStream_t st);

// ---- duplicate groups (vs_components.hip) ---------------------------------------------
// The range scan and the range refine with a union-find in place of the pair buffer (vs_range_scan.h):
// every passing row of query q -- a stored row, self[q], under VS_SELF_ABOVE -- is an edge: cnt[q] += 1
// and the two rows' trees in parent[0, n_valid) are joined, the larger root under the smaller.
hipError_t launch_cc_init(uint32_t* parent, int64_t n, hipStream_t st);  // parent[i] = i
// as launch_range_scan / launch_range_refine; of RangeArgs corpus, d, dpad, dt, metric, n_valid, q, nq,
// radius, go, cnt, self and row0 are read (self_mode must be VS_SELF_ABOVE)
hipError_t launch_cc_scan(const RangeArgs& a, uint32_t* parent, int G, int qy, const uint32_t* ids, int64_t m,
                          hipStream_t st);
hipError_t launch_cc_refine(const RangeArgs& a, uint32_t* parent, const u64* glist, const int* gcnt, int lcap, int ny,
                            hipStream_t st);
// labels[id] = the root of id's tree for the m members: rows sel_ids[0, m) (ascending, each < n), or with
// sel_ids null rows 0..m-1; the caller fills labels[0, n) with -1 first
hipError_t launch_cc_labels(uint32_t* parent, const uint32_t* sel_ids, int64_t m, int64_t n, int64_t* labels,
                            hipStream_t st);

// ---- density clusters (vs_dbscan.hip) -------------------------------------------------
// The self-join of the duplicate groups with one of two sinks (vs_range_scan.h).  deg set: pass 1 -- every
// passing row of query q is an edge: cnt[q] += 1, deg[self[q]] += 1, deg[row] += 1 (deg[0, n_valid), zeroed
// by the caller; an add is not idempotent, so no query may be answered twice).  deg null: pass 2 -- an edge
// between two rows with core[] set joins their trees in parent[0, n_valid); an edge with one core end
// raises best[the other end] to the core row's key; cnt is not written.
struct DbSinkArgs {
    uint32_t* deg;             // pass 1
    uint32_t* parent;          // pass 2 (launch_cc_init first)
    const uint8_t* core;       // pass 2
    unsigned long long* best;  // pass 2 (zeroed by the caller)
};
// as launch_cc_scan / launch_cc_refine
hipError_t launch_db_scan(const RangeArgs& a, const DbSinkArgs& s, int G, int qy, const uint32_t* ids, int64_t m,
                          hipStream_t st);
hipError_t launch_db_refine(const RangeArgs& a, const DbSinkArgs& s, const u64* glist, const int* gcnt, int lcap, int ny,
                            hipStream_t st);
// core[id] = deg[id] + 1 >= min_samples for the m members (as launch_cc_labels names them); the caller zeroes
// core[0, n) first
hipError_t launch_db_core(const uint32_t* deg, const uint32_t* sel_ids, int64_t m, int64_t n, int64_t min_samples,
                          uint8_t* core, hipStream_t st);
// for the m members: degrees[id] = deg[id]; with labels set also labels[id] / kinds[id] = the root of its own
// tree / VS_DBSCAN_CORE for a core row, the root of best[id]'s core row / VS_DBSCAN_BORDER for a row with
// best[id] != 0, -1 / VS_DBSCAN_NOISE for the rest.  The caller fills labels and degrees with -1 and kinds
// with 0 first.
struct DbLabelArgs {
    const uint32_t* deg;
    uint32_t* parent;
    const uint8_t* core;
    const unsigned long long* best;
    const uint32_t* sel_ids;
    int64_t m, n;
    int64_t* labels;
    uint8_t* kinds;
    int64_t* degrees;
};
hipError_t launch_db_labels(const DbLabelArgs& a, hipStream_t st);

// ---- queries taken from stored rows (vs_rows.hip) -----------------------------------------------
// exact lists [nq][kk] (best first, -1 padded) -> [nq][k], k <= kk, with the entry whose id is self[q]
// taken out and the rest moved up; a list that does not hold self[q] keeps its first k entries; slots
// the list cannot fill are padded as vs_search pads them.  Inputs and outputs must not overlap.
struct RowsTakeArgs {
    const int64_t* self;   // [nq] the row each query was gathered from
    const int64_t* I_in;   // [nq][kk]
    const float* D_in;     // [nq][kk]
    const double* S_in;    // [nq][kk] (with S64)
    int kk, k, metric;
    float* D;              // [nq][k]
    int64_t* I;            // [nq][k]
    double* S64;           // [nq][k] (may be null)
};
hipError_t launch_rows_take(const RowsTakeArgs& a, int64_t nq, hipStream_t st);

// ---- k-means over stored rows (vs_kmeans.hip) ---------------------------------------
// mem[i] = sel_ids[i] (null: i) for the m members, ascending
hipError_t launch_km_members(const uint32_t* sel_ids, int64_t m, int64_t* mem, hipStream_t st);
// lab[i] = (int)I[i]; *changed += labels that differ from lab's earlier contents, counts[label] += 1
// (the caller zeroes both first); *bad = 1 if a label lies outside [0, k)
hipError_t launch_km_labels(const int64_t* I, int64_t m, int k, int32_t* lab, unsigned* counts,
                            unsigned long long* changed, int* bad, hipStream_t st);
// part[0, km_obj_blocks(m)) = partial sums of S[0, m) in a fixed order
int km_obj_blocks(int64_t m);
hipError_t launch_km_objsum(const double* S, int64_t m, double* part, hipStream_t st);
// one stable LSD radix pass over bits [shift, shift + 8) of keys_in (vals_in null = positions 0..m-1);
// table: 256 * km_sort_blocks(m) words of scratch.  No atomic decides a slot.
int64_t km_sort_blocks(int64_t m);
hipError_t launch_km_sort_pass(const int32_t* keys_in, const uint32_t* vals_in, int64_t m, int shift, unsigned* table,
                               int32_t* keys_out, uint32_t* vals_out, hipStream_t st);
// P[s][0, d) = the fp64 sum, in order, of rows mem[order[seg[s].x + j]], j < seg[s].y <= VS_KMEANS_SEG,
// read from the tiled layout (one wave per segment and 8 chunk columns); m members, n_valid stored rows
hipError_t launch_km_segsum(int dt, const uint8_t* data, int d, int dpad, const int64_t* mem, const uint32_t* order,
                            const uint2* seg, int64_t nseg, int64_t m, int64_t n_valid, double* P, hipStream_t st);
// cen[c] = (float)((P[segoff[c]] + ... + P[segoff[c + 1] - 1]) / counts[c]); counts[c] == 0: untouched
hipError_t launch_km_finalize(const double* P, const int64_t* segoff, const unsigned* counts, int k, int d, float* cen,
                              hipStream_t st);

// ---- diversified search (vs_diverse.hip) ---------------------------------------------
constexpr int DV_THREADS = 256;           // k_diverse_walk: one workgroup per query
constexpr int DV_BLOCK = 64;              // candidates resolved per step of the walk
constexpr int DV_K_MAX = K_MAX;  // accepted rows kept in LDS (vs_search's k limit)
struct DiverseArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;
    const int64_t* I_in;    // [nq][L] each query's exact ranking, best first (an entry < 0 ends it)
    const float* D_in;      // [nq][L] the scores vs_search reports for them
    int64_t L;              // list length: any
    const float* radius;    // [nq]
    int k;                  // <= DV_K_MAX
    int nqs;                // LDS query slots of a workgroup: diverse_query_slots(d), >= 1
    int64_t* I;            // [nq][k] accepted rows in acceptance order, -1 padded
    float* D;               // [nq][k] their D_in, padded with the worst score
    int32_t* hidden;        // [nq][k] rows hidden under each, 0 padded
    int32_t* nacc;          // [nq] accepted rows
    int64_t* examined;      // [nq] list entries the walk looked at
};
// candidate rows a workgroup stages at a time as fp64 queries (one per wave, as many of the four as
// fit in LDS beside the accepted set); 0: d is too large for the walk (d > 14336)
int diverse_query_slots(int d);
hipError_t launch_diverse_walk(const DiverseArgs& a, int nq, hipStream_t st);

// ---- grouped search (vs_group.hip) ---------------------------------------------------
// A row's group code (vs_groups, gid[row]): >= 0 the dense index of its key among the distinct
// non-negative keys, ascending; < 0 an ungrouped row, ~code its index among the ungrouped keys.
constexpr int GR_THREADS = 64;            // k_group_walk: one wave per query
constexpr int GR_BLOCK = 64;              // candidates loaded per step of the walk
constexpr int GR_K_MAX = K_MAX;  // group slots kept in LDS (vs_search's k limit)
constexpr int GR_TABLE = 8192;            // open-address table of identified groups (>= 2.5 GR_K_MAX)
constexpr int GR_NONE = -0x7FFFFFFF - 1;  // slot_code of an unused slot
struct GroupWalkArgs {
    const int32_t* gid;     // [n_cov] group codes
    int64_t n_cov;          // rows the groups object covers (list entries at or past it are passed over)
    const int64_t* gkey;    // [G] keys of the groups
    const int32_t* gsize;   // [G] members of each group (the object's own sizes, or k_group_count's)
    const int64_t* ukey;    // [U] keys of the ungrouped rows
    int metric;
    const int64_t* I_in;    // [nq][L] each query's exact ranking, best first (an entry < 0 ends it)
    const float* D_in;      // [nq][L] the scores vs_search reports for them
    int64_t L;              // list length: any
    int k, g;               // group slots and member slots per group of the outputs: k * g <= GR_K_MAX
    int k_target;           // groups a walk accepts: 1 .. k
    int64_t* keys;          // [nq][k] group keys in order of first appearance, INT64_MIN padded
    int64_t* I;             // [nq][k][g] members in list order, -1 padded
    float* D;               // [nq][k][g] their D_in, padded with the worst score
    int32_t* found;         // [nq][k] members held, 0 padded
    int32_t* sizes;         // [nq][k] gsize of the group (1 for an ungrouped row), 0 padded
    int32_t* slot_code;     // [nq][k] the group code of each slot, GR_NONE padded
    int32_t* nacc;          // [nq] groups accepted
    int32_t* complete;      // [nq] 1 = k_target groups accepted and each holds min(g, gsize) members
};
hipError_t launch_group_walk(const GroupWalkArgs& a, int nq, hipStream_t st);
// gsize[code] += 1 per listed id below n_cov with a group, cnt[0] += groups that got their first member
// and ungrouped rows listed, cnt[1] += ids below n_cov (gsize [G] and cnt [2] zeroed by the caller)
hipError_t launch_group_count(const int32_t* gid, int64_t n_cov, const uint32_t* ids, int64_t m, int32_t* gsize,
                              unsigned* cnt, hipStream_t st);
// bits[w] (ceil(n_cov / 64) words) = the rows of [0, n_cov) that sel_bits allows (null: every row; rows at
// or past n_sel are not allowed) and whose group's state byte is 1, or 0 while `open`; ungrouped rows
// pass while `open`
hipError_t launch_group_restrict(const int32_t* gid, int64_t n_cov, const uint64_t* sel_bits, int64_t n_sel,
                                 const uint8_t* state, int open, uint64_t* bits, hipStream_t st);
// clears the bits of rows ids[0, n) (each < n_cov)
hipError_t launch_group_clear(uint64_t* bits, int64_t n_cov, const int64_t* ids, int n, hipStream_t st);

// ---- adjusted search (vs_adjust.hip) -------------------------------------------------
// A row's adjusted score is A = fl64(fl64((double)scale[row] * S) + (double)bias[row]), S its canonical
// fp64 score; a row with (scale, bias) = (1, +-0) is plain (A == S bit for bit).
constexpr int AJ_THREADS = 512;           // k_adjust_walk: one workgroup per query
constexpr int AJ_N_MAX = 2 * K_MAX;       // entries of one walk: a list and a scan list of K_MAX each
constexpr size_t AJ_DYN_CAP = 144 * 1024; // its dynamic LDS: the entries' keys and ids, the query as fp64
// what the adjusted scans and the walk read of a vs_adjust (and of the caller's selector)
struct AdjustRows {
    const float* scale;        // [n_cov]
    const float* bias;         // [n_cov]
    int64_t n_cov;             // rows covered: rows at or past it are no members
    const uint64_t* sel_bits;  // the caller's selector (rows at or past n_sel are not allowed), or null
    int64_t n_sel;
};
enum { AJ_PLAIN = 0, AJ_DIRECT = 1, AJ_BOUND = 2 };  // AdjustWalkArgs::mode
struct AdjustWalkArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    AdjustRows rows;        // (sel_bits unused: every entry is a member already)
    const float* q;         // [nq][d] fp32 queries of the launch
    const int64_t* I_list;  // [nq][L] each query's exact plain ranking, best first (an entry < 0 ends it), or null
    int64_t L;
    const int64_t* I_scan;  // [..][ks] adjusted-scan lists, best first, -1 padded; query j's is row qmap[j]; or null
    const int64_t* qmap;    // [nq] (null: the identity)
    int ks;
    int mode;               // AJ_PLAIN: rank every entry, always complete; AJ_DIRECT: the list's adjusted entries
                            // are dropped, complete iff k plain ones are left; AJ_BOUND: complete iff the k-th
                            // best A strictly beats the bound on every row behind the list
    double smin, smax, bmin, bmax;  // AJ_BOUND: the extrema over the covered rows
    int k;
    double* S_tmp;          // [nq][L + ks] scratch: the entries' canonical scores
    int64_t* I;             // [nq][k] rows by (A, id), -1 padded
    float* D;               // [nq][k] (float)A, padded with the worst score
    float* D_raw;           // [nq][k] (float)S, padded alike
    int32_t* complete;      // [nq] (a list shorter than L held every member: complete)
};
size_t adjust_walk_lds(int64_t n_entries, int d);  // dynamic LDS of one walk workgroup
hipError_t launch_adjust_walk(const AdjustWalkArgs& a, int nq, hipStream_t st);
// fs_scan_body ranking by A: ids null = rows [0, a.n_valid) (the caller sets n_valid = rows.n_cov), else
// the m listed rows (ascending; those at or past rows.n_cov, or not allowed by rows.sel_bits, are passed
// over); a.G, qy, a.cert / a.all_queries as in launch_sel_scan.  D / S64 report A.
hipError_t launch_adjust_scan(const FullScanArgs& a, const AdjustRows& rows, const uint32_t* ids, int64_t m, int qy,
                              hipStream_t st);

// ---- fused search (vs_fuse.hip) ------------------------------------------------------
// A fused query is m sub-queries; a row's fused score F is the best (ANY) or the worst (ALL) of its m
// canonical fp64 scores, bit-equal to one of them.
constexpr int FUSE_MAX_Q = 8;                // = VS_FUSE_MAX_Q
constexpr int FUSE_WALK_MAX = 8192;          // = VS_FUSE_WALK_MAX: entries of one walk (m lists of L)
constexpr size_t FUSE_DYN_CAP = 144 * 1024;  // the walk's dynamic LDS: the entries' keys and ids, one sub-query as fp64
enum { FUSE_ANY = 0, FUSE_ALL = 1 };
struct FuseWalkArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;        // rows of the shard: an entry at or past it ends its list like an absent one
    const float* q;         // [nq][m][d] fp32 sub-queries of the launch's fused queries
    int m, mode;            // sub-queries per fused query (1..FUSE_MAX_Q); FUSE_ANY / FUSE_ALL
    const int64_t* I_list;  // [nq][nl][L] lists of row ids, best first (an entry < 0 ends a list)
    int nl;                 // lists per fused query: m (list j is sub-query j's exact ranking) or 1 (a scan's list)
    int64_t L;              // nl * L <= FUSE_WALK_MAX
    int certify;            // 1: complete as the ALL certificate says (nl == m); 0: always complete
    int k;                  // (an answer shorter than k is padded)
    double* S_tmp;          // [nq][nl L][m] scratch: the distinct entries' canonical scores
    uint32_t* E_tmp;        // [nq][nl L] scratch: the distinct entries' ids, ascending
    int64_t* I;             // [nq][k] rows by (F, id), -1 padded
    float* D;               // [nq][k] (float)F, padded with the worst score
    int32_t* which;         // [nq][k] the lowest j with S_j == F, -1 padded
    float* D_sub;           // [nq][k][m] (float)S_j, padded with the worst score
    int32_t* complete;      // [nq]
};
size_t fuse_walk_lds(int64_t n_entries, int d);  // dynamic LDS of one walk workgroup
hipError_t launch_fuse_walk(const FuseWalkArgs& a, int nq, hipStream_t st);
// the streaming scan ranking by F: a.q is [a.nq][m][d], every row scored against the m sub-queries in one
// pass; ids null = rows [0, a.n_valid), else the n_ids listed rows (ascending, each < a.n_valid); a.G
// workgroups split the sequence, qy (1..a.nq) slices deal the fused queries; a.I / a.cert as in
// launch_sel_scan with a.all_queries set (a.D / a.S64 report F where given)
hipError_t launch_fuse_scan(const FullScanArgs& a, int m, int mode, const uint32_t* ids, int64_t n_ids, int qy,
                            hipStream_t st);

// ---- multi-vector search (vs_maxsim.hip) ---------------------------------------------
// A group's score is F = ((M_0 + M_1) + ...) + M_{m-1}, M_j the best canonical fp64 score of a member with
// sub-query j.  A group's code is its index among the distinct non-negative keys, or G + u for the u-th
// ungrouped row: codes [0, ncodes), ncodes = G + U; the member lists are ml_rows [n_cov] (rows by (code,
// id)) and ml_off [ncodes + 1].
struct MaxsimGroups {
    const int32_t* gid;       // [n_cov] group codes as vs_groups keeps them (ungrouped row u: ~u)
    int64_t n_cov, G, ncodes;
    const uint32_t* ml_rows;  // [n_cov]
    const int64_t* ml_off;    // [ncodes + 1]
    const int64_t* gkey;      // [G]
    const int64_t* ukey;      // [U]
};
struct MaxsimWalkArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;
    MaxsimGroups g;
    const uint64_t* sel_bits;  // the members' bitmap over rows [0, n_sel), or null: every covered row
    int64_t n_sel;
    const float* q;         // [nq][m][d] fp32 sub-queries of the launch's queries
    int m;
    const int64_t* cand;    // [nq][nl][L]: row ids, best first (an entry < 0 ends a list), or group codes (codes = 1)
    int nl;                 // m (list j is sub-query j's exact ranking) or 1 (the rank kernel's codes)
    int64_t L;              // nl * L <= FUSE_WALK_MAX
    int codes;              // 1: cand holds group codes; never certified, never capped
    int hold_all;           // 1: the lists held every member: complete whatever the bound says, no row cap
    int64_t walk_rows;      // a query whose candidate groups hold more rows stays open (lists only)
    int k;
    double* M_tmp;          // [nq][nl L][m] scratch: the candidate groups' best scores
    uint32_t* I_tmp;        // [nq][nl L][m] scratch: the lowest member ids that attain them
    uint32_t* C_tmp;        // [nq][nl L] scratch: the distinct candidate codes, ascending
    int32_t* Z_tmp;         // [nq][nl L] scratch: members of each candidate group under the selector
    int64_t* keys;          // [nq][k] group keys, INT64_MIN padded
    double* F;              // [nq][k], padded with -+inf
    float* D_sub;           // [nq][k][m] (float)M_j, padded with the worst score
    int64_t* I_sub;         // [nq][k][m], -1 padded
    int64_t* sizes;         // [nq][k], 0 padded
    int32_t* complete;      // [nq] 1 complete, 0 open (deeper lists may close it), 2 over the row cap (only the scan can)
    int64_t* walked;        // [nq] rows of the candidate groups' member lists
};
size_t maxsim_walk_lds(int64_t n_entries, int d, int m, bool* qlds);  // dynamic LDS of one walk workgroup
hipError_t launch_maxsim_walk(const MaxsimWalkArgs& a, int nq, hipStream_t st);
// the scan: table [nq][m][ncodes] (zeroed) takes the 64-bit maximum of the order-preserving image of every
// member's S_j.  ids null = rows [0, g.n_cov), else the n_ids listed rows (ascending, each < g.n_cov); G
// workgroups split the sequence, qy (1..nq) slices deal the queries.
struct MaxsimScanArgs {
    const uint8_t* corpus;
    int d, dpad, dt, metric;
    MaxsimGroups g;
    const float* q;  // [nq][m][d]
    int nq, m;
    unsigned long long* table;
    int variant;  // measurement only: bit 0 = lane 0 offers every pair, bit 1 = a relaxed load in front of the atomic
};
hipError_t launch_maxsim_scan(const MaxsimScanArgs& a, const uint32_t* ids, int64_t n_ids, int G, int qy, hipStream_t st);
// the rank: per query the k best codes under (F, code) out of the table, as cand [nq][k] (-1 padded)
hipError_t launch_maxsim_rank(const unsigned long long* table, int nq, int m, int64_t ncodes, int metric, int k,
                              int64_t* cand, hipStream_t st);

// ---- paged search (vs_after.hip) -----------------------------------------------------
// A query's cursor is the position (S*, c) in vs_search's total order: c a stored row (or -1: from the
// top), S* its canonical fp64 score with the query.  On the device S* is held as the scan's key, S or -S
// for L2, so "better" is always "greater" (fs_better).
constexpr int AF_THREADS = 256;  // k_after_cut: one workgroup per query
constexpr int AF_D_MAX = 14336;  // the cut kernel stages the query as fp64 in LDS (112 KiB at this d)
struct AfterCursor {
    const int64_t* id;    // [the call's queries] cursor row, -1 = from the top
    const double* key;    // [the call's queries] its key (unused where id is -1)
    const int64_t* qmap;  // [nq of the launch] the call's query behind launch query j (null: the identity)
};
// key[j] = the key of row after[j] with query j (after[j] < 0: 0); one wave per query
hipError_t launch_after_score(int dt, int metric, const uint8_t* corpus, int d, int dpad, int64_t n_valid, const float* q,
                              const int64_t* after, int64_t nq, double* key, hipStream_t st);
struct AfterCutArgs {
    const uint8_t* corpus;  // tiled shard
    int d, dpad, dt, metric;
    int64_t n_valid;        // rows of the shard: an entry at or past it ends the list like an absent one
    const float* q;         // [nq][d] fp32 queries of the launch
    const int64_t* I_list;  // [nq][L] each query's exact ranking among the members, best first (an entry < 0 ends it)
    const float* D_list;    // [nq][L] the scores vs_search reports for them: (float)S
    int64_t L;
    AfterCursor cur;
    int k;
    int64_t* I;             // [nq][k] the list's entries p .. p + k - 1, -1 padded
    float* D;               // [nq][k] their D_list, padded with the worst score
    int64_t* rank;          // [nq] p: the list's entries at or before the cursor
    int32_t* complete;      // [nq] 1: k entries behind the cursor, or the list ended before L (it held every member)
};
hipError_t launch_after_cut(const AfterCutArgs& a, int nq, hipStream_t st);
// fs_scan_body over the rows strictly after each query's cursor: ids null = rows [0, a.n_valid), else the m
// listed rows (ascending, each < a.n_valid); every row of the sequence at or before the cursor is passed
// over and counted into rank[q] (zeroed by the caller); a.G, qy, a.cert / a.all_queries as in
// launch_sel_scan; cur is indexed by the launch's queries through cur.qmap
hipError_t launch_after_scan(const FullScanArgs& a, const AfterCursor& cur, unsigned long long* rank, const uint32_t* ids,
                             int64_t m, int qy, hipStream_t st);

constexpr int I8_GROUP_ROWS = 4096;  // rows per group of the int8 copy's group residuals (16 tiles)
constexpr int I8_MAX_K = 1024;  // largest k the int8 screen serves (k_refine_wide: 2 * KA <= RFW_CAP)
// The index's device words (vs_index::d_maxsq): [0] max ||x||^2, [1] uncertified counter, [2..3] int8
// screen maxima (max ||s c||, max beta; fp32 bits), [4] full-scan counter, [5..6] group residuals
// (max ||mu_g||, groups with a mean), [7] max ||x - s c||, [8] min ||s c|| over the quantised rows
// (fp32 bits, rounded down; +inf while no row is quantised), [9] spare, [10..11] one 64-bit count of
// the rows k_refine_wide scored (vs_refine_rows_count).  The int8 kernels get `maxes` = words 2 on.
constexpr int IX_WORDS = 12;
constexpr int IX_REFINE_ROWS = 10;  // (8-byte aligned)
constexpr int I8_MIN_XH = 6;        // maxes[I8_MIN_XH] = word 8
constexpr unsigned F32_INF_BITS = 0x7F800000u;
// the int8 query credit (vs_set_i8_query_credit): a query whose own int8 error is below the share the
// rows' bound words carry for it gets the difference back in its refine margin (k_pack_qtile_i8)
void set_i8_query_credit(int on);
int i8_query_credit();
// int8 screen copy of stored rows [r0, r0 + n) (maxes[0..1]: running max ||x_hat||, max beta;
// maxes[I8_MIN_XH]: running min ||x_hat||)
hipError_t launch_quant_rows(int dt, const uint8_t* data, int dpad, int64_t r0, int64_t n, int d, uint8_t* data8,
                             int dpad8, uint32_t* rsb, unsigned* maxes, hipStream_t st, const uint16_t* gmean = nullptr);
// group means of the int8 copy (groups [g0, g0 + ng) of I8_GROUP_ROWS rows, rows < n_rows; bf16
// [group][dpad8], zero where the mean is not worth coding against; maxes[0] = max ||mu|| (fp32
// bits), maxes[1] += groups with a mean) and their dots with a query batch (T [group][MFMA_QB])
hipError_t launch_group_means(int dt, const uint8_t* data, int dpad, int d, int64_t g0, int64_t ng, int64_t n_rows,
                              int dpad8, uint16_t* gmean, unsigned* maxes, hipStream_t st);
hipError_t launch_group_dots(const uint16_t* gmean, int64_t ngroups, int dpad8, const float* q, int nq, int d, float* T,
                             hipStream_t st);
// The device fallback round's native query tile, packed ahead by the first pass's query pack (so
// the gated round needs no pack launch of its own): the tile in the corpus dtype (bf16 / f16), its
// qinfo, and zeroed survivor-list lengths / drop bounds of the round's screen.
struct NativeTile {
    int dt;
    int dpad;
    uint8_t* qt;
    float* qinfo;
    int* gcnt;
    u64* drop;
};
hipError_t launch_pack_qtile_i8(const float* q, int nqb, int d, int dpad8, uint8_t* qt, float2* qfac, float* qeps,
                                const unsigned* maxes, int* gcnt, u64* drop, hipStream_t st, int* fails = nullptr,
                                const unsigned* l2max = nullptr, float gamma = 0.0f,
                                const NativeTile* nat = nullptr);

// ---- IVF-Flat (vs_ivf.hip) ---------------------------------------------------------------------
// Inverted lists are chains of pages: a page is one row tile (TR rows, the flat layout above) of
// a shared page pool; storage slot = page * TR + row.  A scan work item is (list, page range,
// up to IVF_QG queries probing that list).
constexpr int IVF_QG = 8;                       // queries per scan item
constexpr int IVF_ITEM_INTS = 4 + IVF_QG;       // list, page_begin, page_end, nq_item, query ids
struct IvfScanArgs {
    const uint8_t* data;       // page pool
    const float* sqn;          // ||x||^2 per slot (L2 screening)
    const float* qp;           // [nq][dpad] fp32 queries (k_pack_qf32)
    const int* items;          // [n_items][IVF_ITEM_INTS]
    int n_items;
    const int* list_pages;     // page table: pages of list l at list_pages[page_off[l] ...]
    const int* page_off;       // [nlist + 1]
    const int64_t* list_n;     // rows per list
    int dpad, metric, Kp, cap;
    u64* cand;                 // [gridDim][nq_item][cap] workspace
    u64* glist;                // per-query candidate lists [nq][lcap] (refine input) ...
    int* gcnt;                 // ... with their lengths (zeroed before the scan)
    int lcap;
    int* next_item;            // k_ivf_scan_dyn: work-queue counter (zeroed before the launch)
};
hipError_t launch_ivf_scan(int dt, int nq_class, const IvfScanArgs& a, int grid, hipStream_t st);
// every class in one launch, items fetched dynamically (nq_class of each item from its query count)
hipError_t launch_ivf_scan_dyn(int dt, const IvfScanArgs& a, int grid, hipStream_t st);
hipError_t launch_round_f32(int dt, float* x, int64_t n, hipStream_t st);  // in place, to the dtype's values
// pack fp32 rows into the slots slots[r] (slot_id[slot] = id0 + r); sqn / maxsq as k_pack_rows
hipError_t launch_pack_rows_map(int dt, const float* src, int64_t n, int d, int dpad, uint8_t* data,
                                const int64_t* slots, float* sqn, unsigned* maxsq, uint32_t* slot_id, int64_t id0,
                                hipStream_t st);

}  // namespace vs

#include <functional>
#include <shared_mutex>
#include <vector>

struct vs_index;
// the owned result of a range search (include/vs.h): query q's rows are [lims[q], lims[q + 1])
struct vs_range_result {
    std::vector<int64_t> lims;
    std::vector<float> D;
    std::vector<int64_t> I;
    std::vector<double> S;  // canonical fp64 scores of the same rows (internal)
};
namespace vs {
// the stored rows of a flat index as the kernels see them; read it (and launch on it) while holding
// flat_lock(ix) shared, the lock adds and resets take exclusively
struct FlatView {
    const uint8_t* data;
    int d, dpad, dtype, metric, device;
    int64_t ntotal;
};
FlatView flat_view(vs_index* ix);
std::shared_mutex& flat_lock(vs_index* ix);
// bumped by vs_reset and by a vs_remove_ids that removed a row: row i of a handle stamped with an
// earlier value (selectors, graphs) is no longer row i
uint64_t flat_generation(vs_index* ix);

// Host <-> HBM row streaming through two pinned host chunks (bulk add, persistence).
// add_rows_host appends n rows: fill(r0, m, dst) writes rows r0..r0+m-1 (fp32, row-major) into a
// pinned chunk while the copy engine and the pack kernel work on the previous one.  Takes the
// index's exclusive lock.
void add_rows_host(vs_index* ix, int64_t n, const std::function<void(int64_t, int64_t, float*)>& fill);
// read_rows_host streams rows i0..i0+n-1 as stored (dtype values widened to fp32): sink(r0, m, src)
// consumes one pinned chunk while the next is unpacked and copied.  Shared lock (concurrent with
// searches).
void read_rows_host(vs_index* ix, int64_t i0, int64_t n,
                    const std::function<void(int64_t, int64_t, const float*)>& sink);
int64_t stream_chunk_rows(int d);  // rows per pinned chunk (32 MiB of fp32)

// Exact top-k of device queries over a flat index, certificate failures re-searched (MFMA dtypes: by
// a gated fallback round on the device, then the gated exact full scan; async = no host sync).
// I_dev [nq][k], S64_dev optional.
// unres (optional): a device counter of this call's queries answered by the full scan, i.e. even
// the fallback round could not certify them (default: the index's counter behind vs_full_scan_count)
void search_exact_device(vs_index* ix, const float* q_dev, int64_t nq, int k, int64_t* I_dev, double* S64_dev,
                         hipStream_t st, float* D_dev = nullptr, int64_t id_offset = 0, bool async = false,
                         unsigned* unres = nullptr);
// drop rows [n, ntotal) of a flat index (rows are append-only: a failed multi-device add rolls back
// the shards that took their rows); the running maxima stay (they only widen certificate margins)
void truncate_rows(vs_index* ix, int64_t n);
unsigned* full_scan_counter(vs_index* ix);  // device word behind vs_full_scan_count
// Exact filtered top-k of device queries (vs_search_sel's tiers; outputs device [nq][k], padded with
// -1 / the worst score past the allowed rows; k may exceed the rows of a non-empty index).  Synchronises `st` (the overfetch tier reads its
// per-query counts back).  Takes the index's shared lock.
void search_sel_device(vs_index* ix, const vs_sel* sel, const float* q_dev, int64_t nq, int k, float* D_dev,
                       int64_t* I_dev, double* S64_dev, hipStream_t st);
// Exact range search of host queries (vs_range_search's body: lock, lease, tiers); the result's ids
// are local row ids, its S the canonical fp64 scores (kept for the multi-device merge).
void range_search_host(vs_index* ix, const vs_sel* sel, const float* q, int64_t nq, const float* radius,
                       int64_t max_total, vs_range_result* out);
// S concurrent exact device searches over parts of one batch (own streams and workspaces;
// unres[i] counts part i's full-scanned queries)
// D_dev / S64_dev (optional): the fp32 and canonical fp64 scores, [nq][k] like I_dev
void search_exact_device_parts(vs_index* ix, const float* q_dev, int64_t nq, int k, int64_t* I_dev,
                               hipStream_t* streams, int S, unsigned* unres, float* D_dev = nullptr,
                               double* S64_dev = nullptr);
// two-phase exact device search (vs_search_device_phase_a / _b)
bool two_phase_ok(const vs_index* ix, int64_t nq, int k);
vs_pending* search_phase_a(vs_index* ix, const float* q_dev, int64_t nq, int k, int world, int64_t id_offset,
                           double* S_a, int64_t* I_a, int stride, hipStream_t st);
// (unres: this call's counter of full-scanned queries, the fallback round could not certify them;
// null = the index's)
void search_phase_b(vs_pending* p, const double* floor_S, float* D, int64_t* I, double* S64, int stride,
                    hipStream_t st, unsigned* unres = nullptr);
void search_pending_free(vs_pending* p);
// seed pass: screen one tile per workgroup (tile_stride) and write per-query 16-row-group maxima
hipError_t launch_seed_mfma(int dt, const ScreenArgs& a, const uint8_t* qt, int nqb, hipStream_t st);
// thr0[q] = key just below the rank-th largest of the M group maxima of query q (0 if none)
hipError_t launch_seed_select(const float* seedmax, int M, int nq, int rank, u64* thr0, hipStream_t st);

hipError_t launch_merge_shards(int metric, const double* S_in, const int64_t* I_in, int G, int64_t nq, int k,
                               double* S_out, int64_t* I_out, float* D_out, hipStream_t st, int istride = 1);

// ---- HNSW graph search (vs_hnsw.hip) ---------------------------------------------
// faiss HNSW::search over a graph in faiss's layout (neighbors of node i on level l:
// neighbors[offsets[i] + cum[l] .. offsets[i] + cum[l + 1]), -1 padded), rows of a flat index,
// canonical fp64 distances.  One workgroup per query; the candidate and result heaps are sorted
// LDS arrays under (distance, id).
constexpr int HN_THREADS = 256;          // k_hnsw_prune: one workgroup per node
constexpr int HN_SEARCH_THREADS = 512;   // k_hnsw_search: one workgroup per query (8 waves score a list)
constexpr int HN_EF_MAX = 2048;  // largest max(efSearch, k)
constexpr int HN_NB_MAX = 1024;  // largest neighbour list of one level
struct HnswArgs {
    const uint8_t* corpus;       // flat index rows (tiled layout)
    int d, dpad, dt, metric;
    int64_t n;                   // rows (= graph nodes)
    const uint64_t* offsets;     // [n + 1]
    const int* neighbors;        // [offsets[n]]
    const int* cum;              // [max_level + 2] cumulative neighbour counts per level
    int entry, max_level;
    int nbmax;                   // widest level's neighbour count
    const float* q;              // [nq][d] fp32
    int k, ef_search, ef;        // ef = max(ef_search, k)
    uint32_t* vis;               // [nq][vis_words] visited bitmaps, zeroed before the launch
    int64_t vis_words;
    float* D;                    // [nq][k] scores (IP) / squared distances (L2), best first
    int64_t* I;                  // [nq][k] row ids, -1 padded
};
size_t hnsw_lds_bytes(int d, int k, int ef, int nbmax);  // dynamic LDS of one search workgroup
hipError_t launch_hnsw_search(const HnswArgs& a, int nq, hipStream_t st);

// faiss HNSW::shrink_neighbor_list per node (graph build): one workgroup per node
constexpr int HP_C_MAX = 2048;  // largest candidate list of one node
struct HnswPruneArgs {
    const uint8_t* corpus;  // flat index rows (tiled layout)
    int d, dpad, dt, metric;
    const int64_t* nodes;   // [m] row ids
    const int* cand;        // [m][C] distinct candidate row ids, -1 padded at the end
    int C, W;               // candidates per node, neighbours kept
    int* out;               // [m][W] kept ids best first, -1 padded
};
size_t hnsw_prune_lds_bytes(int d, int C, int W);
hipError_t launch_hnsw_prune(const HnswPruneArgs& a, int m, hipStream_t st);

}  // namespace vs
