// vs_kmeans.hip -- exact k-means over stored rows (include/vs.h "k-means over stored rows").
//
// faiss::Clustering keeps its training rows on the host and sums them there.  Here the members are
// rows the index already holds in HBM (256-row chunk-major tiles), and every step of an iteration
// runs on the device:
//   * assignment: the members are gathered as fp32 queries in chunks (launch_gather_rows) and
//     searched at k = 1 against a temporary fp32 index of the centroids (search_exact_device_parts:
//     every query certified on the device, ties to the lower centroid id); labels, fp32 and fp64
//     scores land in device arrays of m entries;
//   * grouping: k_km_labels narrows the labels, counts the changes against the previous pass and
//     the members per cluster (integer atomics: the counts do not depend on their order); a stable
//     LSD radix sort on the label, 8 bits a pass (k_km_hist, k_km_scan, k_km_scatter), orders the
//     member positions by (label, id).  The rank of an element inside its block comes from wave
//     ballots and per-wave counts in LDS, never from an atomic;
//   * update: a cluster's members in that order are cut into segments of VS_KMEANS_SEG.  k_km_segsum
//     gives each wave one (segment, 8 chunk columns) task: lane l owns the 16 B piece l & 7 of chunk
//     l >> 3 -- 4 fp32 or 8 bf16 / f16 columns, one fp64 accumulator each -- so a wave instruction
//     reads eight whole 128 B lines of one member row, eight members' loads are in flight per lane,
//     and the adds run in member order.  k_km_finalize adds a cluster's partials in segment order,
//     divides and rounds.  The adds are __dadd_rn, the division __ddiv_rn: nothing to contract or
//     reassociate, so the centroids are a pure function of the inputs.
// Every store is bounded: sort outputs by m, partials by nseg x d, centroids by k x d.  Plain vector
// stores only.
#include "vs_index.h"
#include "vs_device.h"
#include "vs_dispatch.h"

using namespace vs;

namespace vs {

constexpr int KM_THREADS = 256;
constexpr int KM_NW = KM_THREADS / 64;
constexpr int KM_TILE = 2048;  // elements one workgroup of the radix sort ranks (8 rounds of 256)
constexpr int KM_U = 8;        // member rows whose loads a lane of k_km_segsum keeps in flight
constexpr int KM_CG = 8;       // chunk columns per k_km_segsum task (64 lanes x 16 B = 8 lines)
constexpr int KM_OBJ_BLOCKS = 256;

// ids of the members, ascending: the selector's list, or 0..m-1
__global__ void __launch_bounds__(KM_THREADS) k_km_members(const uint32_t* __restrict__ sel_ids, int64_t m,
                                                           int64_t* __restrict__ mem) {
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (i < m) mem[i] = sel_ids ? (int64_t)sel_ids[i] : i;
}

// lab[i] <- (int)I[i]; *changed += labels that differ from the previous pass; counts[label] += 1;
// a label outside [0, k) sets *bad (and counts as label 0, so nothing downstream indexes past k)
__global__ void __launch_bounds__(KM_THREADS) k_km_labels(const int64_t* __restrict__ I, int64_t m, int k,
                                                          int32_t* __restrict__ lab, unsigned* __restrict__ counts,
                                                          unsigned long long* __restrict__ changed,
                                                          int* __restrict__ bad) {
    const int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    bool diff = false;
    if (i < m) {
        int64_t l = I[i];
        if (l < 0 || l >= k) {
            *bad = 1;
            l = 0;
        }
        diff = lab[i] != (int32_t)l;
        lab[i] = (int32_t)l;
        atomicAdd(&counts[l], 1u);
    }
    const u64 b = __ballot(diff);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(changed, (unsigned long long)__popcll(b));
}

// part[b] = sum of S[i] over the block's grid-stride elements (fixed order: reproducible, though the
// objective's order is free)
__global__ void __launch_bounds__(KM_THREADS) k_km_objsum(const double* __restrict__ S, int64_t m,
                                                          double* __restrict__ part) {
    __shared__ double ws[KM_NW];
    double a = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; i < m; i += (int64_t)gridDim.x * KM_THREADS)
        a += S[i];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) a += __shfl_xor(a, s, 64);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < KM_NW; ++w) t += ws[w];
        part[blockIdx.x] = t;
    }
}

// radix pass, step 1: table[digit * nblocks + b] = elements of block b's tile with that digit
__global__ void __launch_bounds__(KM_THREADS) k_km_hist(const int32_t* __restrict__ keys, int64_t m, int shift,
                                                        unsigned* __restrict__ table, int nblocks) {
    __shared__ unsigned h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * KM_TILE;
    for (int r = 0; r < KM_TILE / KM_THREADS; ++r) {
        const int64_t i = i0 + r * KM_THREADS + threadIdx.x;
        if (i < m) atomicAdd(&h[((unsigned)keys[i] >> shift) & 255u], 1u);  // (a count: order-free)
    }
    __syncthreads();
    table[(int64_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

// radix pass, step 2: exclusive prefix sum of the n table entries in place (one workgroup)
__global__ void __launch_bounds__(1024) k_km_scan(unsigned* __restrict__ t, int64_t n) {
    __shared__ unsigned wsum[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned carry = 0u;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const unsigned v = i < n ? t[i] : 0u;
        unsigned x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o, 64);
            if (lane >= o) x += y;
        }
        if (lane == 63) wsum[w] = x;
        __syncthreads();
        if (w == 0) {
            unsigned s = lane < 16 ? wsum[lane] : 0u;
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                const unsigned y = __shfl_up(s, o, 64);
                if (lane >= o) s += y;
            }
            if (lane < 16) wsum[lane] = s;
        }
        __syncthreads();
        const unsigned woff = w > 0 ? wsum[w - 1] : 0u;
        if (i < n) t[i] = carry + woff + x - v;
        carry += wsum[15];
        __syncthreads();  // (wsum is rewritten by the next chunk)
    }
}

// radix pass, step 3: stable scatter.  An element's slot = the scanned table entry of (its digit,
// this block) + the elements of the block before it with the same digit: those of earlier rounds
// (lbase grows round by round), of earlier waves of this round (wcnt) and of lower lanes of its wave
// (ballots over the digit's bits).  vals_in null = the element's own position.
__global__ void __launch_bounds__(KM_THREADS) k_km_scatter(const int32_t* __restrict__ keys_in,
                                                           const uint32_t* __restrict__ vals_in, int64_t m, int shift,
                                                           const unsigned* __restrict__ table, int nblocks,
                                                           int32_t* __restrict__ keys_out,
                                                           uint32_t* __restrict__ vals_out) {
    __shared__ unsigned lbase[256];
    __shared__ unsigned wcnt[KM_NW][256];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    lbase[threadIdx.x] = table[(int64_t)threadIdx.x * nblocks + blockIdx.x];
#pragma unroll
    for (int j = 0; j < KM_NW; ++j) wcnt[j][threadIdx.x] = 0u;
    __syncthreads();
    const int64_t i0 = (int64_t)blockIdx.x * KM_TILE;
    for (int r = 0; r < KM_TILE / KM_THREADS; ++r) {
        if (i0 + (int64_t)r * KM_THREADS >= m) break;  // (uniform over the workgroup)
        const int64_t i = i0 + r * KM_THREADS + threadIdx.x;
        const bool valid = i < m;
        const int32_t key = valid ? keys_in[i] : 0;
        const unsigned dg = ((unsigned)key >> shift) & 255u;
        u64 same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (dg >> bit) & 1u;
            const u64 bb = __ballot(on);
            same &= on ? bb : ~bb;
        }
        const unsigned rank = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank == 0u) wcnt[w][dg] = (unsigned)__popcll(same);
        __syncthreads();
        if (valid) {
            unsigned off = lbase[dg] + rank;
            for (int j = 0; j < w; ++j) off += wcnt[j][dg];
            if ((int64_t)off < m) {
                keys_out[off] = key;
                vals_out[off] = vals_in ? vals_in[i] : (uint32_t)i;
            }
        }
        __syncthreads();
        unsigned t = 0u;
#pragma unroll
        for (int j = 0; j < KM_NW; ++j) {
            t += wcnt[j][threadIdx.x];
            wcnt[j][threadIdx.x] = 0u;
        }
        lbase[threadIdx.x] += t;
        __syncthreads();
    }
}

// Segment sums.  One wave per (segment, group of KM_CG chunk columns): segment s holds the members at
// positions order[seg[s].x .. + seg[s].y) of the sorted order (1..VS_KMEANS_SEG of one cluster, ascending
// id).  P[s][col] = (((+0.0 + x_0) + x_1) + ...) in fp64, columns < d.  m: members; n_valid: stored rows.
template <int DT>
__global__ void __launch_bounds__(KM_THREADS) k_km_segsum(const uint8_t* __restrict__ data, int d, int dpad,
                                                          const int64_t* __restrict__ mem,
                                                          const uint32_t* __restrict__ order,
                                                          const uint2* __restrict__ seg, int64_t nseg, int ngroups,
                                                          int64_t m, int64_t n_valid, double* __restrict__ P) {
    constexpr int ES = DT == DT_F32 ? 4 : 2;
    constexpr int CE = CHB / ES;   // elements of a chunk
    constexpr int EPL = 16 / ES;   // columns a lane owns
    const int lane = threadIdx.x & 63;
    const int64_t task = (int64_t)blockIdx.x * KM_NW + (threadIdx.x >> 6);
    const int64_t s = task / ngroups;
    if (s >= nseg) return;  // (uniform over the wave)
    const int cg = (int)(task % ngroups);
    const int c = cg * KM_CG + (lane >> 3), piece = lane & 7;
    const bool cvalid = c < dpad / CE;
    const int64_t coff = (int64_t)c * TR * CHB + piece * 16;
    const uint2 sg = seg[s];
    const int len = (int)sg.y;
    double acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.0;
    for (int j0 = 0; j0 < len; j0 += 64) {
        const int nb = min(64, len - j0);
        // the rows of up to 64 members, one per lane (ids < 2^32); positions and ids are bounded here
        // as well, so that no load leaves the member list or the stored rows
        int rowv = 0;
        if (lane < nb && (int64_t)sg.x + j0 + lane < m) {
            const uint32_t pos = order[(int64_t)sg.x + j0 + lane];
            const int64_t id = (int64_t)pos < m ? mem[pos] : 0;
            rowv = id >= 0 && id < n_valid ? (int)(uint32_t)id : 0;
        }
        for (int u0 = 0; u0 < nb; u0 += KM_U) {
            uint4 raw[KM_U];
#pragma unroll
            for (int u = 0; u < KM_U; ++u) {
                const int64_t r = (int64_t)(uint32_t)__shfl(rowv, u0 + u, 64);
                raw[u] = make_uint4(0u, 0u, 0u, 0u);
                if (u0 + u < nb && cvalid)
                    raw[u] = *(const uint4*)(data + (r / TR) * (int64_t)TR * dpad * ES + (r % TR) * CHB + coff);
            }
#pragma unroll
            for (int u = 0; u < KM_U; ++u) {
                if (u0 + u < nb) {  // (uniform over the wave)
                    float x[EPL];
                    unpack16<DT>(raw[u], x);
#pragma unroll
                    for (int e = 0; e < EPL; ++e) acc[e] = __dadd_rn(acc[e], (double)x[e]);
                }
            }
        }
    }
    if (cvalid) {
        const int col0 = c * CE + piece * EPL;
#pragma unroll
        for (int e = 0; e < EPL; ++e)
            if (col0 + e < d) P[s * d + col0 + e] = acc[e];
    }
}

// centroid c, column col: the cluster's partials added in segment order, divided by its member
// count and rounded to fp32; an empty cluster keeps its centroid
__global__ void __launch_bounds__(KM_THREADS) k_km_finalize(const double* __restrict__ P,
                                                            const int64_t* __restrict__ segoff,
                                                            const unsigned* __restrict__ counts, int k, int d,
                                                            float* __restrict__ cen) {
    const int64_t idx = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x;
    if (idx >= (int64_t)k * d) return;
    const int c = (int)(idx / d), col = (int)(idx % d);
    const unsigned n = counts[c];
    if (n == 0u) return;
    double sum = 0.0;
    for (int64_t s = segoff[c]; s < segoff[c + 1]; ++s) sum = __dadd_rn(sum, P[s * d + col]);
    cen[idx] = (float)__ddiv_rn(sum, (double)n);
}

static inline unsigned km_blocks(int64_t n) { return (unsigned)((n + KM_THREADS - 1) / KM_THREADS); }

hipError_t launch_km_members(const uint32_t* sel_ids, int64_t m, int64_t* mem, hipStream_t st) {
    if (m <= 0 || !mem || (m + KM_THREADS - 1) / KM_THREADS > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_members, dim3(km_blocks(m)), dim3(KM_THREADS), 0, st, sel_ids, m, mem);
    return hipGetLastError();
}

hipError_t launch_km_labels(const int64_t* I, int64_t m, int k, int32_t* lab, unsigned* counts,
                            unsigned long long* changed, int* bad, hipStream_t st) {
    if (m <= 0 || k <= 0 || !I || !lab || !counts || !changed || !bad ||
        (m + KM_THREADS - 1) / KM_THREADS > 0x7FFFFFFF)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_labels, dim3(km_blocks(m)), dim3(KM_THREADS), 0, st, I, m, k, lab, counts, changed, bad);
    return hipGetLastError();
}

int km_obj_blocks(int64_t m) { return (int)std::min<int64_t>(KM_OBJ_BLOCKS, (m + KM_THREADS - 1) / KM_THREADS); }

hipError_t launch_km_objsum(const double* S, int64_t m, double* part, hipStream_t st) {
    if (m <= 0 || !S || !part) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_objsum, dim3((unsigned)km_obj_blocks(m)), dim3(KM_THREADS), 0, st, S, m, part);
    return hipGetLastError();
}

int64_t km_sort_blocks(int64_t m) { return (m + KM_TILE - 1) / KM_TILE; }

// one stable radix pass on bits [shift, shift + 8) of the keys; table: 256 * km_sort_blocks(m) words
hipError_t launch_km_sort_pass(const int32_t* keys_in, const uint32_t* vals_in, int64_t m, int shift, unsigned* table,
                               int32_t* keys_out, uint32_t* vals_out, hipStream_t st) {
    const int64_t nb = km_sort_blocks(m);
    if (m <= 0 || !keys_in || !keys_out || !vals_out || !table || shift < 0 || shift > 24 || nb > 0x7FFFFF)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_hist, dim3((unsigned)nb), dim3(KM_THREADS), 0, st, keys_in, m, shift, table, (int)nb);
    hipLaunchKernelGGL(k_km_scan, dim3(1), dim3(1024), 0, st, table, 256 * nb);
    hipLaunchKernelGGL(k_km_scatter, dim3((unsigned)nb), dim3(KM_THREADS), 0, st, keys_in, vals_in, m, shift,
                       (const unsigned*)table, (int)nb, keys_out, vals_out);
    return hipGetLastError();
}

hipError_t launch_km_segsum(int dt, const uint8_t* data, int d, int dpad, const int64_t* mem, const uint32_t* order,
                            const uint2* seg, int64_t nseg, int64_t m, int64_t n_valid, double* P, hipStream_t st) {
    const int ce = CHB / es_of(dt);
    if (!data || !mem || !order || !seg || !P || nseg <= 0 || d <= 0 || dpad < d || dpad % ce != 0 || m <= 0 ||
        n_valid < m)
        return hipErrorInvalidValue;
    const int ngroups = (dpad / ce + KM_CG - 1) / KM_CG;
    const int64_t blocks = (nseg * ngroups + KM_NW - 1) / KM_NW;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 g((unsigned)blocks), b(KM_THREADS);
    const bool known = with_dt(dt, [&](auto dt_c) {
        launch_kernel(k_km_segsum<dt_c>, 0, g, b, 0, st, data, d, dpad, mem, order, seg, nseg, ngroups, m, n_valid, P);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_km_finalize(const double* P, const int64_t* segoff, const unsigned* counts, int k, int d, float* cen,
                              hipStream_t st) {
    const int64_t blocks = ((int64_t)k * d + KM_THREADS - 1) / KM_THREADS;
    if (!P || !segoff || !counts || !cen || k <= 0 || d <= 0 || blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_finalize, dim3((unsigned)blocks), dim3(KM_THREADS), 0, st, P, segoff, counts, k, d, cen);
    return hipGetLastError();
}

}  // namespace vs

namespace {

constexpr int64_t kDefaultKmeansStaging = 256ll << 20;
std::atomic<int64_t> g_kmeans_staging{kDefaultKmeansStaging};

// the last vs_kmeans call of the process: ms spent in assignment, grouping and update (HIP events on
// the call's stream), passes and updates run (vs_kmeans_last_times)
std::mutex g_times_mu;
double g_times[5] = {0, 0, 0, 0, 0};

constexpr int kParts = 8;  // concurrent searches of the centroid index (as the IVF coarse assignment)

// the streams and events of one call, destroyed with it
struct KmStreams {
    hipStream_t main = nullptr, part[kParts] = {};
    DevEvent fork, join[kParts], t[4];
    void create() {
        HIP_CHECK(hipStreamCreateWithFlags(&main, hipStreamNonBlocking));
        for (hipStream_t& s : part) HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        fork.create(hipEventDisableTiming);
        for (DevEvent& e : join) e.create(hipEventDisableTiming);
        for (DevEvent& e : t) e.create();
    }
    ~KmStreams() {
        if (main) (void)hipStreamDestroy(main);
        for (hipStream_t s : part)
            if (s) (void)hipStreamDestroy(s);
    }
};

// the temporary centroid index, destroyed with the call
struct TmpIndex {
    vs_index* h = nullptr;
    ~TmpIndex() { vs_destroy(h); }
};

void check_rc(int rc) {
    if (rc != VS_OK) throw VsError(rc, std::string("centroid index: ") + vs_last_error());
}

}  // namespace

extern "C" {

int vs_set_kmeans_staging_bytes(int64_t bytes) {
    return guarded([&] {
        if (bytes < 1) throw VsError(VS_ERR_ARG, "k-means staging bytes must be >= 1 (the floor is one 256-row block)");
        g_kmeans_staging.store(bytes);
    });
}

int vs_kmeans_last_times(double* out, int cap) {
    return guarded([&] {
        if (!out || cap < 0) throw VsError(VS_ERR_ARG, "null buffer");
        std::lock_guard<std::mutex> g(g_times_mu);
        for (int i = 0; i < std::min(cap, 5); ++i) out[i] = g_times[i];
    });
}

int vs_kmeans(vs_index* index, const vs_sel* sel, int32_t k, int32_t niter, int32_t metric, float* centroids,
              int64_t* labels, float* D, int64_t* counts, double* objective, int64_t* changed, int32_t* iters_done) {
    vs_index* ix = index;
    return guarded([&] {
        check_index(ix);
        if (metric == -1) metric = ix->metric;
        if (metric != VS_METRIC_IP && metric != VS_METRIC_L2)
            throw VsError(VS_ERR_ARG, "metric must be VS_METRIC_IP, VS_METRIC_L2 or -1 (the index's)");
        if (k < 1) throw VsError(VS_ERR_ARG, "k must be >= 1");
        if (niter < 0) throw VsError(VS_ERR_ARG, "niter must be >= 0");
        if (!centroids || !labels) throw VsError(VS_ERR_ARG, "centroids and labels must not be null");
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        if (sel) check_sel(ix, sel);
        const int64_t m = sel ? sel->m : ix->ntotal;
        if (m == 0) {  // nothing to assign: pass 0 of no members, no update
            if (counts) std::fill(counts, counts + k, (int64_t)0);
            if (objective) objective[0] = 0.0;
            if (changed) changed[0] = 0;
            if (iters_done) *iters_done = 0;
            return;
        }
        if (k > m) throw VsError(VS_ERR_ARG, "k = " + std::to_string(k) + " exceeds the " + std::to_string(m) + " members");
        DeviceGuard dg(ix->device);
        const int d = ix->d;
        // ---- workspace (counted in vs_device_bytes_live, freed as the call returns) ----
        const int64_t chunk = std::min(round_up(m, MFMA_QB),
                                       std::max<int64_t>(g_kmeans_staging.load() / ((int64_t)d * 4) / MFMA_QB, 1) * MFMA_QB);
        const int passes = [&] {
            int bits = 0;
            while (bits < 31 && (1ll << bits) < (int64_t)k) ++bits;
            return std::max(1, (bits + 7) / 8);
        }();
        const int64_t sort_words = 256 * km_sort_blocks(m);
        DevBuf cen, qbuf, mem, I64, Dd, Sd, lab, cnt, misc, keys[2], vals[2], table, segs, segoff, P;
        cen.ensure((size_t)k * d * sizeof(float));
        qbuf.ensure((size_t)chunk * d * sizeof(float));
        mem.ensure((size_t)m * sizeof(int64_t));
        I64.ensure((size_t)m * sizeof(int64_t));
        Dd.ensure((size_t)m * sizeof(float));
        Sd.ensure((size_t)m * sizeof(double));
        lab.ensure((size_t)m * sizeof(int32_t));
        cnt.ensure((size_t)k * sizeof(unsigned));
        // misc: [0] changed (u64), [1] bad label flag (int, padded), [2..] objective partials
        misc.ensure((size_t)(2 + KM_OBJ_BLOCKS) * 8);
        if (niter > 0) {
            for (int b = 0; b < 2; ++b) {
                keys[b].ensure((size_t)m * sizeof(int32_t));
                vals[b].ensure((size_t)m * sizeof(uint32_t));
            }
            table.ensure((size_t)sort_words * sizeof(unsigned));
            segoff.ensure((size_t)(k + 1) * sizeof(int64_t));
        }
        KmStreams S;
        S.create();
        hipStream_t st = S.main;
        TmpIndex tmp;
        check_rc(vs_create(d, metric, VS_DTYPE_F32, ix->device, &tmp.h));
        std::vector<unsigned> cnt_h((size_t)k);
        std::vector<int64_t> segoff_h((size_t)k + 1);
        std::vector<uint2> seg_h;
        std::vector<uint64_t> misc_h((size_t)2 + KM_OBJ_BLOCKS);
        double ms[3] = {0, 0, 0};
        int updates = 0, t = 0;
        try {
            HIP_CHECK(hipMemcpyAsync(cen.p, centroids, (size_t)k * d * sizeof(float), hipMemcpyHostToDevice, st));
            HIP_CHECK(launch_km_members(sel ? sel->ids : nullptr, m, mem.as<int64_t>(), st));
            HIP_CHECK(hipMemsetAsync(lab.p, 0xFF, (size_t)m * sizeof(int32_t), st));  // pass -1: no label
            HIP_CHECK(hipStreamSynchronize(st));
            for (;; ++t) {
                // ---- assignment pass t ----
                check_rc(vs_reset(tmp.h));
                check_rc(vs_add_device(tmp.h, cen.as<float>(), k, st));
                HIP_CHECK(hipEventRecord(S.t[0], st));
                for (int64_t q0 = 0; q0 < m; q0 += chunk) {
                    const int64_t c = std::min(chunk, m - q0);
                    HIP_CHECK(launch_gather_rows(ix->dtype, ix->data, mem.as<int64_t>() + q0, c, d, ix->dpad,
                                                 qbuf.as<float>(), st));
                    HIP_CHECK(hipEventRecord(S.fork, st));
                    for (int i = 0; i < kParts; ++i) HIP_CHECK(hipStreamWaitEvent(S.part[i], S.fork, 0));
                    search_exact_device_parts(tmp.h, qbuf.as<float>(), c, 1, I64.as<int64_t>() + q0, S.part, kParts,
                                              nullptr, Dd.as<float>() + q0, Sd.as<double>() + q0);
                    for (int i = 0; i < kParts; ++i) {
                        HIP_CHECK(hipEventRecord(S.join[i], S.part[i]));
                        HIP_CHECK(hipStreamWaitEvent(st, S.join[i], 0));
                    }
                }
                HIP_CHECK(hipEventRecord(S.t[1], st));
                // ---- labels, changes, counts, objective ----
                HIP_CHECK(hipMemsetAsync(cnt.p, 0, (size_t)k * sizeof(unsigned), st));
                HIP_CHECK(hipMemsetAsync(misc.p, 0, 16, st));
                HIP_CHECK(launch_km_labels(I64.as<int64_t>(), m, k, lab.as<int32_t>(), cnt.as<unsigned>(),
                                           misc.as<unsigned long long>(), (int*)(misc.as<uint64_t>() + 1), st));
                HIP_CHECK(launch_km_objsum(Sd.as<double>(), m, (double*)(misc.as<uint64_t>() + 2), st));
                HIP_CHECK(hipMemcpyAsync(misc_h.data(), misc.p, misc_h.size() * 8, hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipMemcpyAsync(cnt_h.data(), cnt.p, (size_t)k * sizeof(unsigned), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
                {
                    float a = 0.0f;
                    HIP_CHECK(hipEventElapsedTime(&a, S.t[0], S.t[1]));
                    ms[0] += a;
                }
                if ((int)(misc_h[1] & 0xFFFFFFFFu) != 0) throw VsError(VS_ERR_INTERNAL, "k-means: assignment out of range");
                const int64_t nchanged = (int64_t)misc_h[0];
                if (changed) changed[t] = nchanged;
                if (objective) {
                    double o = 0.0;
                    for (int b = 0; b < km_obj_blocks(m); ++b) {
                        double v;
                        std::memcpy(&v, &misc_h[(size_t)2 + b], 8);
                        o += v;
                    }
                    objective[t] = o;
                }
                if ((t >= 1 && nchanged == 0) || t == niter) break;
                // ---- update t: order the members by (label, id), segment sums, new centroids ----
                const int32_t* kin = lab.as<int32_t>();
                const uint32_t* vin = nullptr;
                for (int p = 0; p < passes; ++p) {
                    HIP_CHECK(launch_km_sort_pass(kin, vin, m, 8 * p, table.as<unsigned>(), keys[p & 1].as<int32_t>(),
                                                  vals[p & 1].as<uint32_t>(), st));
                    kin = keys[p & 1].as<int32_t>();
                    vin = vals[p & 1].as<uint32_t>();
                }
                // segments: cluster c's members are the sorted positions [start_c, start_c + count_c)
                seg_h.clear();
                int64_t start = 0;
                for (int c = 0; c < k; ++c) {
                    segoff_h[(size_t)c] = (int64_t)seg_h.size();
                    for (int64_t o = 0; o < (int64_t)cnt_h[(size_t)c]; o += VS_KMEANS_SEG)
                        seg_h.push_back(make_uint2((unsigned)(start + o),
                                                   (unsigned)std::min<int64_t>(VS_KMEANS_SEG, cnt_h[(size_t)c] - o)));
                    start += cnt_h[(size_t)c];
                }
                segoff_h[(size_t)k] = (int64_t)seg_h.size();
                if (start != m) throw VsError(VS_ERR_INTERNAL, "k-means: cluster counts do not add up to the members");
                const int64_t nseg = (int64_t)seg_h.size();
                segs.ensure((size_t)nseg * sizeof(uint2));
                P.ensure((size_t)nseg * d * sizeof(double));
                HIP_CHECK(hipMemcpyAsync(segs.p, seg_h.data(), (size_t)nseg * sizeof(uint2), hipMemcpyHostToDevice, st));
                HIP_CHECK(hipMemcpyAsync(segoff.p, segoff_h.data(), (size_t)(k + 1) * sizeof(int64_t),
                                         hipMemcpyHostToDevice, st));
                HIP_CHECK(hipEventRecord(S.t[2], st));
                HIP_CHECK(launch_km_segsum(ix->dtype, ix->data, d, ix->dpad, mem.as<int64_t>(), vin, segs.as<uint2>(), nseg,
                                           m, ix->ntotal, P.as<double>(), st));
                HIP_CHECK(launch_km_finalize(P.as<double>(), segoff.as<int64_t>(), cnt.as<unsigned>(), k, d, cen.as<float>(),
                                             st));
                HIP_CHECK(hipEventRecord(S.t[3], st));
                HIP_CHECK(hipStreamSynchronize(st));  // (seg_h / segoff_h are reused; the index refill reads cen)
                {  // grouping: from the end of the searches (labels, the host's segment list included)
                    float a = 0.0f, b = 0.0f;
                    HIP_CHECK(hipEventElapsedTime(&a, S.t[1], S.t[2]));
                    HIP_CHECK(hipEventElapsedTime(&b, S.t[2], S.t[3]));
                    ms[1] += a;
                    ms[2] += b;
                }
                ++updates;
            }
            // ---- results of the last pass, and the centroids it was run against ----
            HIP_CHECK(hipMemcpyAsync(labels, I64.p, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            if (D) HIP_CHECK(hipMemcpyAsync(D, Dd.p, (size_t)m * sizeof(float), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if (updates > 0) {
                HIP_CHECK(hipMemcpyAsync(centroids, cen.p, (size_t)k * d * sizeof(float), hipMemcpyDeviceToHost, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
        } catch (...) {
            (void)hipDeviceSynchronize();  // the buffers are freed behind the queued work
            throw;
        }
        if (counts)
            for (int c = 0; c < k; ++c) counts[c] = (int64_t)cnt_h[(size_t)c];
        if (iters_done) *iters_done = updates;
        {
            std::lock_guard<std::mutex> g(g_times_mu);
            g_times[0] = ms[0];
            g_times[1] = ms[1];
            g_times[2] = ms[2];
            g_times[3] = t + 1;
            g_times[4] = updates;
        }
    });
}

}  // extern "C"
