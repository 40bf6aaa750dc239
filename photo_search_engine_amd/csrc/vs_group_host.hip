// vs_group_host.hip -- host side of the grouped search (include/vs.h "grouped search"; kernels:
// vs_group.hip).
//
// A walk over a list that is a prefix of a query's exact ranking identifies groups in their true order
// (every row not in the list ranks below every row in it), so it is complete once it holds `target`
// groups with min(g, members of the group) rows each, or once the list held every member.  Tiers:
//   1  the exact top-L0 of every query (exact_lists, valid on the device), walked on the device;
//   2  the queries not complete re-searched at 4 L, up to the limit, and walked again from scratch;
//      (tiers 1 and 2 are deepen_lists of vs_walk.h, shared with the diversified search)
//   3  restricted rounds, one query at a time: the member set cut down on the device to the rows of the
//      identified groups still short of members and -- while fewer than `target` groups are identified
//      -- of the groups not yet seen, compacted into a temporary selector, ranked by the filtered
//      search's own road at depth min(limit, rows left), walked from scratch and merged on the host.
// Removing rows does not reorder the rest, so a round's list starts with the rows of its set the list
// before it held: an identified group's new member list has its old one as a prefix, and new groups
// appear behind every identified one, in true order.  A list that does not hold its whole set holds
// limit >= k g rows: a row of a group not yet seen identifies that group; otherwise they are rows of at
// most k short groups, one of which then has g of them and completes.
#include "vs_walk.h"

using namespace vs;

namespace {

constexpr int64_t kKeyPad = -0x7FFFFFFFFFFFFFFFll - 1;  // INT64_MIN: the key of an unused group slot

enum { T_RESTRICT = 6, T_COMPACT = 7 };  // the restricted rounds' own slots of WalkTimes::ms

// the member sets a call works on: the selector the lists are searched under (null: every stored row),
// the members of each group and the number of groups that have one
struct GrMembers {
    const vs_sel* sel = nullptr;
    int64_t members = 0, groups = 0;
    const int32_t* gsize = nullptr;  // device [G]
};

// where one call's answers go (found / sizes / codes always exist here; the caller's may be null)
struct GrOut {
    int k, g;
    int64_t* keys;
    float* D;
    int64_t* I;
    std::vector<int32_t> found, sizes, code;  // [nq][k]
    std::vector<int32_t> nacc, complete;      // [nq]
};

// a walk's block for m queries with kk slots of g entries, on the device and copied to the host:
// [keys int64 mk | I int64 mkg | D fp32 mkg | found, sizes, code int32 mk | nacc, complete int32 m]
struct GrBlock {
    int64_t *keys, *I;
    float* D;
    int32_t *found, *sizes, *code, *nacc, *complete;
    size_t bytes;
};
GrBlock gr_block(const void* base, size_t m, size_t mk, size_t mkg) {
    Carver c(base);  // (a braced list is evaluated left to right: the order of the members)
    GrBlock b{c.take<int64_t>(mk), c.take<int64_t>(mkg), c.take<float>(mkg), c.take<int32_t>(mk), c.take<int32_t>(mk),
              c.take<int32_t>(mk), c.take<int32_t>(m), c.take<int32_t>(m)};
    b.bytes = c.used;
    return b;
}

// the walk over m device lists [m][L] with kk slots of g entries and k_target groups to accept; returns
// its results on the host, in h
GrBlock walk_lists(const vs_index* ix, Ctx* c, const vs_groups* gr, const int32_t* gsize, const int64_t* Id,
                   const float* Dd, int64_t L, int64_t m, int kk, int g, int k_target, std::vector<uint8_t>& h,
                   hipStream_t st, DevEvent* ev_done) {
    const size_t mk = (size_t)m * kk, mkg = mk * g;
    const size_t bytes = gr_block(nullptr, m, mk, mkg).bytes;
    c->gr_out.ensure(bytes);
    const GrBlock dev = gr_block(c->gr_out.p, m, mk, mkg);
    GroupWalkArgs a{};
    a.gid = gr->gid.as<int32_t>();
    a.n_cov = gr->n_cov;
    a.gkey = gr->gkey.as<int64_t>();
    a.gsize = gsize;
    a.ukey = gr->ukey.as<int64_t>();
    a.metric = ix->metric;
    a.L = L;
    a.k = kk;
    a.g = g;
    a.k_target = k_target;
    const int64_t qmax = 65536;  // workgroups of one launch
    for (int64_t q0 = 0; q0 < m; q0 += qmax) {
        const int nq = (int)std::min(qmax, m - q0);
        a.I_in = Id + q0 * L;
        a.D_in = Dd + q0 * L;
        a.keys = dev.keys + q0 * kk;
        a.I = dev.I + q0 * kk * g;
        a.D = dev.D + q0 * kk * g;
        a.found = dev.found + q0 * kk;
        a.sizes = dev.sizes + q0 * kk;
        a.slot_code = dev.code + q0 * kk;
        a.nacc = dev.nacc + q0;
        a.complete = dev.complete + q0;
        HIP_CHECK(launch_group_walk(a, nq, st));
    }
    if (ev_done) HIP_CHECK(hipEventRecord(*ev_done, st));
    h.resize(bytes);
    HIP_CHECK(hipMemcpyAsync(h.data(), c->gr_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return gr_block(h.data(), m, mk, mkg);
}

// a tier-1/2 walk's m answers into rows idx[j] of the call's outputs (every slot is written)
void deliver_walk(const GrBlock& w, int64_t m, const int64_t* idx, GrOut& out) {
    const int k = out.k;
    const int64_t kg = (int64_t)k * out.g;
    for (int64_t j = 0; j < m; ++j) {
        const int64_t r = idx[j];
        std::copy(w.keys + j * k, w.keys + (j + 1) * k, out.keys + r * k);
        std::copy(w.I + j * kg, w.I + (j + 1) * kg, out.I + r * kg);
        std::copy(w.D + j * kg, w.D + (j + 1) * kg, out.D + r * kg);
        std::copy(w.found + j * k, w.found + (j + 1) * k, out.found.begin() + r * k);
        std::copy(w.sizes + j * k, w.sizes + (j + 1) * k, out.sizes.begin() + r * k);
        std::copy(w.code + j * k, w.code + (j + 1) * k, out.code.begin() + r * k);
        out.nacc[(size_t)r] = w.nacc[j];
        out.complete[(size_t)r] = w.complete[j];
    }
}

// ---- tier 3: one query's restricted rounds ---------------------------------------------------------
struct Round3 {
    vs_index* ix;
    Ctx* c;
    const vs_groups* gr;
    const GrMembers& mb;
    const vs_sel* user_sel;  // the caller's selector (its bits restrict every round), or null
    int64_t limit;
    int target;
    hipStream_t st;
    TempSel R;
    DevBuf state_d, clear_d;
    std::vector<uint8_t> state_h;
    std::vector<int64_t> clear_h;
    DevEvent e0{hipEventDefault}, e1{hipEventDefault}, e2{hipEventDefault}, e3{hipEventDefault}, e4{hipEventDefault};
};

// returns the rounds run
int64_t restricted_rounds(Round3& r, const float* q, int64_t qi, GrOut& out, WalkTimes& times, int64_t& longest) {
    vs_index* ix = r.ix;
    const vs_groups* gr = r.gr;
    const int k = out.k, g = out.g;
    const int64_t kg = (int64_t)k * g;
    int64_t* keys = out.keys + qi * k;
    int64_t* I = out.I + qi * kg;
    float* D = out.D + qi * kg;
    int32_t* found = out.found.data() + qi * k;
    int32_t* sizes = out.sizes.data() + qi * k;
    int32_t* code = out.code.data() + qi * k;
    int identified = out.nacc[(size_t)qi];
    const int64_t nwords = (gr->n_cov + 63) / 64;
    r.R.bits.ensure((size_t)nwords * 8);
    r.state_h.resize((size_t)std::max<int64_t>(gr->G, 1));
    r.state_d.ensure(r.state_h.size());
    std::vector<uint8_t> h;
    std::vector<int> inc;  // the slots of the identified groups still short of members
    int64_t rounds = 0;
    for (;;) {
        inc.clear();
        for (int s = 0; s < identified; ++s)
            if (found[s] < std::min(g, sizes[s])) inc.push_back(s);
        const bool open = identified < r.target;
        if (inc.empty() && !open) break;
        // the restricted set: state 1 = short of members, 2 = done with (complete, or never wanted), 0 =
        // not yet seen
        std::fill(r.state_h.begin(), r.state_h.end(), (uint8_t)(open ? 0 : 2));
        r.clear_h.clear();
        for (int s = 0; s < identified; ++s) {
            if (code[s] >= 0) r.state_h[(size_t)code[s]] = 2;
            else if (open) r.clear_h.push_back(I[(int64_t)s * g]);  // an identified ungrouped row
        }
        for (int s : inc)
            if (code[s] >= 0) r.state_h[(size_t)code[s]] = 1;  // (an ungrouped row is never short)
        HIP_CHECK(hipEventRecord(r.e0, r.st));
        HIP_CHECK(hipMemcpyAsync(r.state_d.p, r.state_h.data(), r.state_h.size(), hipMemcpyHostToDevice, r.st));
        HIP_CHECK(launch_group_restrict(gr->gid.as<int32_t>(), gr->n_cov, r.user_sel ? r.user_sel->bits : nullptr,
                                        r.user_sel ? r.user_sel->n_sel : 0, r.state_d.as<uint8_t>(), open ? 1 : 0,
                                        r.R.bits.as<uint64_t>(), r.st));
        if (!r.clear_h.empty()) {
            r.clear_d.ensure(r.clear_h.size() * sizeof(int64_t));
            HIP_CHECK(hipMemcpyAsync(r.clear_d.p, r.clear_h.data(), r.clear_h.size() * sizeof(int64_t),
                                     hipMemcpyHostToDevice, r.st));
            HIP_CHECK(launch_group_clear(r.R.bits.as<uint64_t>(), gr->n_cov, r.clear_d.as<int64_t>(), (int)r.clear_h.size(),
                                         r.st));
        }
        HIP_CHECK(hipEventRecord(r.e1, r.st));
        r.R.compact(ix, gr->n_cov, r.mb.members, r.st);
        HIP_CHECK(hipEventRecord(r.e2, r.st));
        const int64_t nR = r.R.s.m;
        if (nR == 0) break;  // (nothing left to rank: every group that has a member is identified and full)
        ++rounds;
        const int kk = (int)std::min<int64_t>(r.limit, nR);
        const int kprime = (int)inc.size() + (r.target - identified);
        stage_queries(ix, r.c, q, qi, 1, r.st);
        const StagedOut so = exact_lists(ix, r.c, &r.R.s, sel_plan(ix, &r.R.s, 1, kk), 1, kk, LISTS_DEVICE, r.st);
        HIP_CHECK(hipEventRecord(r.e3, r.st));
        const GrBlock w = walk_lists(ix, r.c, gr, r.mb.gsize, so.Id, so.Dd, kk, 1, kprime, g, kprime, h, r.st, &r.e4);
        times.ms[T_RESTRICT] += ms_between(r.e0, r.e1);
        times.ms[T_COMPACT] += ms_between(r.e1, r.e2);
        times.search(2) += ms_between(r.e0, r.e3);
        times.walk(2) += ms_between(r.e3, r.e4);
        longest = std::max<int64_t>(longest, kk);
        // merge: an identified group takes the new member list (the old one is its prefix); new groups
        // follow in their order of appearance
        const int before_id = identified;
        int64_t before_rows = 0, after_rows = 0;
        for (int s : inc) before_rows += found[s];
        for (int j = 0; j < w.nacc[0]; ++j) {
            int s = -1;
            if (w.code[j] >= 0)
                for (int t : inc)
                    if (code[t] == w.code[j]) {
                        s = t;
                        break;
                    }
            if (s < 0) {
                if (identified >= r.target) throw VsError(VS_ERR_INTERNAL, "grouped search: a round found too many groups");
                s = identified++;
                keys[s] = w.keys[j];
                sizes[s] = w.sizes[j];
                code[s] = w.code[j];
            } else if (w.found[j] < found[s]) {
                throw VsError(VS_ERR_INTERNAL, "grouped search: a round lost members of a group");
            }
            found[s] = w.found[j];
            std::copy(w.I + (int64_t)j * g, w.I + (int64_t)(j + 1) * g, I + (int64_t)s * g);
            std::copy(w.D + (int64_t)j * g, w.D + (int64_t)(j + 1) * g, D + (int64_t)s * g);
        }
        for (int s : inc) after_rows += found[s];
        if (kk >= nR) break;  // the list held the whole restricted set
        if (identified == before_id && after_rows == before_rows)
            throw VsError(VS_ERR_INTERNAL, "grouped search: a restricted round made no progress");
    }
    out.nacc[(size_t)qi] = identified;
    return rounds;
}

}  // namespace

// (declared in vs_index.h)
void vs::check_groups(const vs_index* ix, const vs_groups* gr) {
    if (!gr) throw VsError(VS_ERR_ARG, "null groups");
    if (gr->ix != ix) throw VsError(VS_ERR_ARG, "groups belong to another index");
    if (gr->gen != ix->reset_gen.load() || gr->n_cov > ix->ntotal)
        throw VsError(VS_ERR_ARG, "stale groups (the index was reset, or rows were removed, after they were made)");
}

extern "C" {

int vs_groups_create(vs_index* ix, const int64_t* keys, int64_t n, vs_groups** out) {
    return guarded([&] {
        if (!out) throw VsError(VS_ERR_ARG, "out is null");
        *out = nullptr;
        check_index(ix);
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        DeviceGuard dg(ix->device);
        if (n != ix->ntotal) throw VsError(VS_ERR_ARG, "group keys: one key per row, n must equal ntotal");
        if (n > 0 && !keys) throw VsError(VS_ERR_ARG, "group keys are null");
        if (n >= 0x7FFFFFFFll) throw VsError(VS_ERR_ARG, "group codes are 32-bit");
        std::unique_ptr<vs_groups, void (*)(vs_groups*)> gr(new vs_groups(), vs_groups_destroy);
        gr->ix = ix;
        gr->gen = ix->reset_gen.load();
        gr->device = ix->device;
        gr->n_cov = n;
        if (n > 0) {
            // the dense index of each row's key among the distinct non-negative keys, ascending
            std::vector<uint32_t> order;
            std::vector<int32_t> gid((size_t)n);
            std::vector<int64_t> gkey, ukey;
            std::vector<int32_t> gsize;
            for (int64_t i = 0; i < n; ++i) {
                if (keys[i] >= 0) {
                    order.push_back((uint32_t)i);
                } else {
                    gid[(size_t)i] = ~(int32_t)ukey.size();
                    ukey.push_back(keys[i]);
                }
            }
            std::sort(order.begin(), order.end(),
                      [&](uint32_t a, uint32_t b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a < b; });
            for (uint32_t i : order) {
                if (gkey.empty() || gkey.back() != keys[i]) {
                    gkey.push_back(keys[i]);
                    gsize.push_back(0);
                }
                gid[i] = (int32_t)gkey.size() - 1;
                ++gsize.back();
            }
            gr->G = (int64_t)gkey.size();
            gr->U = (int64_t)ukey.size();
            gr->gid.ensure((size_t)n * sizeof(int32_t));
            gr->gkey.ensure((size_t)std::max<int64_t>(gr->G, 1) * sizeof(int64_t));
            gr->gsize.ensure((size_t)std::max<int64_t>(gr->G, 1) * sizeof(int32_t));
            gr->ukey.ensure((size_t)std::max<int64_t>(gr->U, 1) * sizeof(int64_t));
            HIP_CHECK(hipMemcpy(gr->gid.p, gid.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
            if (gr->G) {
                HIP_CHECK(hipMemcpy(gr->gkey.p, gkey.data(), (size_t)gr->G * sizeof(int64_t), hipMemcpyHostToDevice));
                HIP_CHECK(hipMemcpy(gr->gsize.p, gsize.data(), (size_t)gr->G * sizeof(int32_t), hipMemcpyHostToDevice));
            }
            if (gr->U)
                HIP_CHECK(hipMemcpy(gr->ukey.p, ukey.data(), (size_t)gr->U * sizeof(int64_t), hipMemcpyHostToDevice));
        }
        *out = gr.release();
    });
}

void vs_groups_destroy(vs_groups* gr) {
    if (!gr) return;
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != gr->device) (void)hipSetDevice(gr->device);
    gr->gid.release();
    gr->gkey.release();
    gr->gsize.release();
    gr->ukey.release();
    gr->ml_rows.release();
    gr->ml_off.release();
    if (prev >= 0 && prev != gr->device) (void)hipSetDevice(prev);
    delete gr;
}

int64_t vs_groups_count(const vs_groups* gr) { return gr ? gr->G : -1; }
int64_t vs_groups_rows(const vs_groups* gr) { return gr ? gr->n_cov : -1; }

int vs_groups_keys(const vs_groups* gr, int64_t* out) {
    return guarded([&] {
        if (!gr) throw VsError(VS_ERR_ARG, "null groups");
        if (gr->G == 0) return;
        if (!out) throw VsError(VS_ERR_ARG, "null host buffer");
        DeviceGuard dg(gr->device);
        HIP_CHECK(hipMemcpy(out, gr->gkey.p, (size_t)gr->G * sizeof(int64_t), hipMemcpyDeviceToHost));
    });
}

int vs_search_groups(vs_index* ix, const vs_groups* gr, const vs_sel* sel, const float* q, int64_t nq, int32_t k,
                     int32_t group_size, int64_t* keys_out, float* D, int64_t* I, int32_t* found_out, int64_t* sizes_out) {
    return guarded([&] {
        check_index(ix);
        const int kmax = K_MAX;
        const int g = group_size;
        if (nq < 0) throw VsError(VS_ERR_ARG, "nq must be >= 0");
        if (k < 1) throw VsError(VS_ERR_ARG, "k must be >= 1");
        if (g < 1) throw VsError(VS_ERR_ARG, "group_size must be >= 1");
        if ((int64_t)k * g > kmax) throw VsError(VS_ERR_ARG, "k * group_size must be <= " + std::to_string(kmax));
        std::shared_lock<std::shared_mutex> lk(ix->rw);
        check_groups(ix, gr);
        if (sel) check_sel(ix, sel);
        const int64_t kg = (int64_t)k * g;
        const WalkState::Depth depth = ix->gr.resolve(std::max<int64_t>(4 * kg, 64), kmax);
        const int64_t limit = depth.limit;
        if (kg > limit)
            throw VsError(VS_ERR_ARG, "k * group_size must be <= the depth limit (vs_set_group_depth): every restricted "
                                      "round needs a list of k * group_size rows to make progress");
        int64_t stats[6] = {nq, 0, 0, 0, 0, 0};
        WalkTimes times;
        auto note = [&] { ix->gr.note(stats, 6, times.ms, 8); };
        if (nq == 0) {
            note();
            return;
        }
        if (!q || !keys_out || !D || !I) throw VsError(VS_ERR_ARG, "null host buffer");
        fill_padding(D, I, nq * kg, worst_score(ix));
        std::fill(keys_out, keys_out + nq * k, kKeyPad);
        GrOut out{k, g, keys_out, D, I, std::vector<int32_t>((size_t)nq * k, 0), std::vector<int32_t>((size_t)nq * k, 0),
                  std::vector<int32_t>((size_t)nq * k, GR_NONE), std::vector<int32_t>((size_t)nq, 0),
                  std::vector<int32_t>((size_t)nq, 0)};
        auto deliver = [&] {
            if (found_out) std::copy(out.found.begin(), out.found.end(), found_out);
            if (sizes_out) std::copy(out.sizes.begin(), out.sizes.end(), sizes_out);
        };
        if (gr->n_cov == 0 || (sel && sel->m == 0)) {  // nothing to rank: all padding
            stats[1] = nq;
            deliver();
            note();
            return;
        }
        DeviceGuard dg(ix->device);
        CtxLease lease(ix, nullptr, true);
        Ctx* c = lease.c;
        hipStream_t st = c->stream;
        // ---- the member set: the covered rows, under the selector those of them it allows -------------
        GrMembers mb;
        TempSel cover;  // the selector cut to the covered rows, when rows were added behind the groups
        DevBuf cnt_sizes;
        if (!sel && gr->n_cov == ix->ntotal) {
            mb.members = gr->n_cov;
            mb.groups = gr->G + gr->U;
            mb.gsize = gr->gsize.as<int32_t>();
        } else {
            mb.sel = sel;
            if (!sel || sel->n_sel > gr->n_cov) {
                cover.cover(ix, sel, gr->n_cov, st);
                mb.sel = &cover.s;
            }
            // members of every group and the groups that have one: [gsize int32 G | cnt unsigned 2]
            const size_t cnt_off = (size_t)round_up(std::max<int64_t>(gr->G, 1) * (int64_t)sizeof(int32_t), 8);
            cnt_sizes.ensure(cnt_off + 2 * sizeof(unsigned));
            HIP_CHECK(hipMemsetAsync(cnt_sizes.p, 0, cnt_off + 2 * sizeof(unsigned), st));
            unsigned* cnt_d = (unsigned*)((uint8_t*)cnt_sizes.p + cnt_off);
            HIP_CHECK(launch_group_count(gr->gid.as<int32_t>(), gr->n_cov, mb.sel->ids, mb.sel->m, cnt_sizes.as<int32_t>(),
                                         cnt_d, st));
            unsigned cnt_h[2] = {0, 0};
            HIP_CHECK(hipMemcpyAsync(cnt_h, cnt_d, sizeof(cnt_h), hipMemcpyDeviceToHost, st));
            HIP_CHECK(hipStreamSynchronize(st));
            if ((int64_t)cnt_h[1] != mb.sel->m) throw VsError(VS_ERR_INTERNAL, "grouped search: member count mismatch");
            mb.members = mb.sel->m;
            mb.groups = cnt_h[0];
            mb.gsize = cnt_sizes.as<int32_t>();
        }
        if (mb.members == 0) {
            stats[1] = nq;
            deliver();
            note();
            return;
        }
        const int target = (int)std::min<int64_t>(k, mb.groups);
        // ---- tiers 1 and 2: exact top-L lists, walked on the device; not complete goes deeper --------
        std::vector<uint8_t> h;
        const Deepened dl = deepen_lists(
            ix, c, st, mb.sel, mb.members, depth.first, limit, q, nq, times,
            [&](const StagedOut& so, int64_t L, int64_t m, const int64_t* idx, DevEvent* ev) {
                deliver_walk(walk_lists(ix, c, gr, mb.gsize, so.Id, so.Dd, L, m, k, g, target, h, st, ev), m, idx, out);
            },
            [&](int64_t r) { return out.complete[(size_t)r] != 0; });
        stats[1] = dl.done[0];
        stats[2] = dl.done[1];
        stats[5] = dl.longest;
        // ---- tier 3: restricted rounds, one query at a time -------------------------------------------
        if (!dl.pending.empty()) {
            Round3 r3{ix, c, gr, mb, sel, limit, target, st};
            for (int64_t qi : dl.pending) {
                stats[4] += restricted_rounds(r3, q, qi, out, times, stats[5]);
                ++stats[3];
            }
        }
        deliver();
        note();
    });
}

int vs_set_group_depth(vs_index* ix, int32_t first, int32_t limit) {
    return guarded([&] {
        check_index(ix);
        ix->gr.set(first, limit, K_MAX, "group");
    });
}

int vs_group_last_stats(vs_index* ix, int64_t* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->gr.mu, ix->gr.stats, 6, out, cap, "stats");
    });
}

int vs_group_last_times(vs_index* ix, double* out, int cap) {
    return guarded([&] {
        check_index(ix);
        copy_last(ix->gr.mu, ix->gr.times, 8, out, cap, "times");
    });
}

}  // extern "C"
