// vs_group.hip -- the kernels of the grouped search (include/vs.h "grouped search"; host:
// vs_group_host.hip).
//
// k_group_walk: one wave per query goes through a list that is a prefix of the query's exact ranking
// (row ids, best first, of any length) and collects the first k_target groups in order of first
// appearance with the first min(g, size) rows of each.  The list is walked in blocks of GR_BLOCK
// candidates: every lane gathers its candidate's group code (4 bytes), and what acceptance would need
// (the group's key and size), into LDS; lane 0 then resolves the block in list order on LDS data alone
// -- two rows of one new group, or a group filling up mid-block, make the order matter -- probing an
// open-address table of the identified groups (linear probing, GR_TABLE slots for at most GR_K_MAX
// groups).  An identified group with room takes the row as its next member; a new group is accepted
// while fewer than k_target are; anything else is passed over.  Ungrouped rows never enter the table:
// each is a group of one.  The walk stops at the first row after which k_target groups are accepted and
// every one of them is full.  The work is L table probes per query and no scoring.
// Every store is bounded: the outputs by k slots of g entries of the query's rows (slot < k_target <= k,
// position < min(g, size) <= g), the LDS arrays by GR_K_MAX, GR_TABLE and GR_BLOCK.  Plain vector stores.
//
// k_group_count: the members of every group, and the groups that have one, under a selector's id list
// (integer atomics: the values do not depend on the order).
// k_group_restrict / k_group_clear: the bitmap of a restricted round's member set.
#include "vs_device.h"

namespace vs {

static_assert(GR_BLOCK == 64 && GR_THREADS == 64, "k_group_walk: one lane per candidate of a block");
static_assert((GR_TABLE & (GR_TABLE - 1)) == 0 && GR_TABLE >= 2 * GR_K_MAX && GR_K_MAX < 0xFFFF, "k_group_walk: table");
constexpr unsigned GR_FREE = 0xFFFFu;

__device__ __forceinline__ unsigned gr_hash(int code) { return ((unsigned)code * 2654435761u) >> 19 & (GR_TABLE - 1); }

__global__ void __launch_bounds__(GR_THREADS) k_group_walk(GroupWalkArgs a) {
    __shared__ uint16_t s_tab[GR_TABLE];   // slot of an identified group (GR_FREE: none)
    __shared__ int s_code[GR_K_MAX];       // group code of each slot
    __shared__ uint16_t s_cnt[GR_K_MAX];   // members held
    __shared__ uint16_t s_need[GR_K_MAX];  // min(g, size)
    __shared__ int64_t s_cid[GR_BLOCK];    // the block's candidate ids
    __shared__ int64_t s_ckey[GR_BLOCK];   // ... the keys of their groups
    __shared__ int s_cg[GR_BLOCK];         // ... their group codes (GR_NONE: no member)
    __shared__ int s_csz[GR_BLOCK];        // ... their groups' sizes
    __shared__ float s_cd[GR_BLOCK];       // ... their scores
    __shared__ int s_nk, s_nfull, s_stop;
    const int64_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const int k = a.k, g = a.g, kt = a.k_target;
    const int64_t* Iq = a.I_in + q * a.L;
    const float* Dq = a.D_in + q * a.L;
    int64_t* Ko = a.keys + q * k;
    int64_t* Io = a.I + q * (int64_t)k * g;
    float* Do = a.D + q * (int64_t)k * g;
    for (int i = tid; i < GR_TABLE; i += GR_THREADS) s_tab[i] = (uint16_t)GR_FREE;
    if (tid == 0) {
        s_nk = 0;
        s_nfull = 0;
        s_stop = 0;
    }
    __syncthreads();
    for (int64_t b0 = 0; b0 < a.L; b0 += GR_BLOCK) {
        int64_t id = b0 + tid < a.L ? Iq[b0 + tid] : -1;
        const u64 ok = __ballot(id >= 0);  // the list ends at its first absent entry
        const int nb = ~ok ? __ffsll((long long)~ok) - 1 : GR_BLOCK;
        if (nb == 0) break;
        int code = GR_NONE, sz = 1;
        int64_t key = 0;
        if (tid < nb && id < a.n_cov) {
            code = a.gid[id];
            if (code >= 0) {
                key = a.gkey[code];
                sz = a.gsize[code];
            } else {
                key = a.ukey[~code];
            }
        }
        s_cid[tid] = id;
        s_cg[tid] = code;
        s_ckey[tid] = key;
        s_csz[tid] = sz;
        s_cd[tid] = tid < nb ? Dq[b0 + tid] : 0.0f;
        __syncthreads();
        if (tid == 0) {  // the block in list order
            int nk = s_nk, nfull = s_nfull;
            for (int c = 0; c < nb; ++c) {
                const int gc = s_cg[c];
                if (gc == GR_NONE) continue;
                int slot;
                unsigned t = GR_FREE;  // the table's entry for the group (GR_FREE: a new group)
                if (gc >= 0) {
                    unsigned h = gr_hash(gc);
                    while ((t = s_tab[h]) != GR_FREE && s_code[t] != gc) h = (h + 1) & (GR_TABLE - 1);
                    if (t != GR_FREE) {
                        slot = (int)t;
                        if (s_cnt[slot] >= s_need[slot]) continue;  // (full: passed over)
                    } else {
                        if (nk >= kt) continue;
                        slot = nk++;
                        s_tab[h] = (uint16_t)slot;
                    }
                } else {
                    if (nk >= kt) continue;
                    slot = nk++;
                }
                if (t == GR_FREE) {  // a new group: slot < kt <= k <= GR_K_MAX
                    const int size = s_csz[c];
                    s_code[slot] = gc;
                    s_cnt[slot] = 0;
                    s_need[slot] = (uint16_t)(size < g ? size : g);
                    Ko[slot] = s_ckey[c];
                    a.sizes[q * k + slot] = size;
                    a.slot_code[q * k + slot] = gc;
                }
                const int pos = s_cnt[slot];  // < need <= g (0 for a new group)
                s_cnt[slot] = (uint16_t)(pos + 1);
                Io[(int64_t)slot * g + pos] = s_cid[c];
                Do[(int64_t)slot * g + pos] = s_cd[c];
                if (pos + 1 == s_need[slot]) ++nfull;
                if (nk == kt && nfull == nk) {
                    s_stop = 1;
                    break;
                }
            }
            s_nk = nk;
            s_nfull = nfull;
        }
        __syncthreads();
        if (s_stop || nb < GR_BLOCK) break;
    }
    __syncthreads();
    const int nk = s_nk;
    const float worst = a.metric == METRIC_L2 ? 3.402823466e+38f : -3.402823466e+38f;
    for (int e = tid; e < k * g; e += GR_THREADS) {
        const int slot = e / g, pos = e - slot * g;
        if (slot >= nk || pos >= s_cnt[slot]) {
            Io[e] = -1;
            Do[e] = worst;
        }
    }
    for (int j = tid; j < k; j += GR_THREADS) {
        if (j < nk) {
            a.found[q * k + j] = s_cnt[j];
        } else {
            Ko[j] = (int64_t)(-0x7FFFFFFFFFFFFFFFll - 1);
            a.found[q * k + j] = 0;
            a.sizes[q * k + j] = 0;
            a.slot_code[q * k + j] = GR_NONE;
        }
    }
    if (tid == 0) {
        a.nacc[q] = nk;
        a.complete[q] = (nk == kt && s_nfull == nk) ? 1 : 0;
    }
}

hipError_t launch_group_walk(const GroupWalkArgs& a, int nq, hipStream_t st) {
    if (nq <= 0) return hipSuccess;
    if (a.k < 1 || a.g < 1 || (int64_t)a.k * a.g > GR_K_MAX || a.k_target < 1 || a.k_target > a.k || a.L < 1 ||
        a.n_cov < 0 || !a.gid || !a.I_in || !a.D_in || !a.keys || !a.I || !a.D || !a.found || !a.sizes || !a.slot_code ||
        !a.nacc || !a.complete || (a.metric != METRIC_IP && a.metric != METRIC_L2))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_walk, dim3(nq), dim3(GR_THREADS), 0, st, a);
    return hipGetLastError();
}

constexpr int GC_THREADS = 256;

__global__ void __launch_bounds__(GC_THREADS) k_group_count(const int32_t* __restrict__ gid, int64_t n_cov,
                                                            const uint32_t* __restrict__ ids, int64_t m,
                                                            int32_t* __restrict__ gsize, unsigned* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * GC_THREADS + threadIdx.x;
    bool member = false, first = false;
    if (i < m) {
        const int64_t id = ids[i];
        if (id < n_cov) {
            member = true;
            const int code = gid[id];
            first = code < 0 || atomicAdd(&gsize[code], 1) == 0;
        }
    }
    const int nm = __popcll(__ballot(member)), nf = __popcll(__ballot(first));
    if ((threadIdx.x & 63) == 0) {
        if (nf) atomicAdd(&cnt[0], (unsigned)nf);
        if (nm) atomicAdd(&cnt[1], (unsigned)nm);
    }
}

hipError_t launch_group_count(const int32_t* gid, int64_t n_cov, const uint32_t* ids, int64_t m, int32_t* gsize,
                              unsigned* cnt, hipStream_t st) {
    if (m <= 0) return hipSuccess;
    const int64_t G = (m + GC_THREADS - 1) / GC_THREADS;
    if (!gid || !ids || !cnt || n_cov < 0 || G > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_count, dim3((unsigned)G), dim3(GC_THREADS), 0, st, gid, n_cov, ids, m, gsize, cnt);
    return hipGetLastError();
}

// one lane per row, one ballot per word: lane l of a wave owns bit l of word (row >> 6)
__global__ void __launch_bounds__(GC_THREADS) k_group_restrict(const int32_t* __restrict__ gid, int64_t n_cov,
                                                               const u64* __restrict__ sel_bits, int64_t n_sel,
                                                               const uint8_t* __restrict__ state, int open,
                                                               u64* __restrict__ bits) {
    const int64_t i = (int64_t)blockIdx.x * GC_THREADS + threadIdx.x;
    bool in = false;
    if (i < n_cov) {
        in = !sel_bits || (i < n_sel && ((sel_bits[i >> 6] >> (i & 63)) & 1ull));
        if (in) {
            const int code = gid[i];
            const int s = code >= 0 ? state[code] : 0;
            in = s == 1 || (s == 0 && open);
        }
    }
    const u64 w = __ballot(in);
    if ((threadIdx.x & 63) == 0 && (i >> 6) < ((n_cov + 63) >> 6)) bits[i >> 6] = w;
}

hipError_t launch_group_restrict(const int32_t* gid, int64_t n_cov, const uint64_t* sel_bits, int64_t n_sel,
                                 const uint8_t* state, int open, uint64_t* bits, hipStream_t st) {
    if (n_cov <= 0) return hipSuccess;
    const int64_t G = (n_cov + GC_THREADS - 1) / GC_THREADS;
    if (!gid || !bits || G > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_restrict, dim3((unsigned)G), dim3(GC_THREADS), 0, st, gid, n_cov, (const u64*)sel_bits,
                       n_sel, state, open, (u64*)bits);
    return hipGetLastError();
}

__global__ void __launch_bounds__(GC_THREADS) k_group_clear(u64* __restrict__ bits, int64_t n_cov,
                                                            const int64_t* __restrict__ ids, int n) {
    const int i = blockIdx.x * GC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id >= 0 && id < n_cov) atomicAnd((unsigned long long*)&bits[id >> 6], ~(1ull << (id & 63)));
}

hipError_t launch_group_clear(uint64_t* bits, int64_t n_cov, const int64_t* ids, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (!bits || !ids) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_group_clear, dim3((n + GC_THREADS - 1) / GC_THREADS), dim3(GC_THREADS), 0, st, (u64*)bits,
                       n_cov, ids, n);
    return hipGetLastError();
}

}  // namespace vs
