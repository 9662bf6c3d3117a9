// Host-side structure pass of the pose-graph solver (pgo.hip): junctions, segments and the index lists the kernels walk.
// Plain C++ without HIP, so that it can also be compiled into a stand-alone program and run under host sanitizers.
//
// A pose graph is a few odometry chains plus loop closures.  A JUNCTION is the prior pose or any pose whose number of
// distinct neighbours is not 2; a SEGMENT is a maximal path of non-junction poses (its interior) with the two junctions at
// its ends.  Interiors are eliminated as block-tridiagonal systems, the junctions are left in one dense system.  A cycle
// without a junction gets its lowest pose promoted; an interior longer than PGO_SEG_MAX is cut by promoting every
// (PGO_SEG_MAX + 1)-th pose of it, which bounds the sequential depth of the elimination.  Parallel edges between the same
// two poses share one off-diagonal block.  The plan is a pure function of its input: every list is built in index order.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

#define PGO_SEG_MAX 64            // poses in one segment interior at most (sequential depth of the block recurrence)
#define PGO_MAX_JUNCTIONS 4096    // dense junction system: (6 J)^2 doubles = 4.8 GB at the cap

#define PGO_PLAN_E_ARG (-1)       // an index out of range, or an edge with i == j
#define PGO_PLAN_E_LIMIT (-2)     // more junctions than PGO_MAX_JUNCTIONS

// kinds of a segment's contribution to a block of the junction system (a, b = its end junctions)
#define PGO_KIND_AA 0
#define PGO_KIND_BB 1
#define PGO_KIND_AB 2
#define PGO_KIND_BA 3             // AB transposed

struct PgoPlan {
    int64_t n = 0, nf = 0;                 // poses; between factors (the prior is factor nf)
    int32_t prior = 0;
    // unique pose pairs (pa < pb), sorted; the factors of a pair in ascending order as fac * 2 + (1 when the factor's i > j)
    std::vector<int32_t> pa, pb, pair_ptr, pair_fac;
    // the factors incident to a pose in ascending order as fac * 4 + role (0: the pose is i, 1: it is j, 2: the prior)
    std::vector<int32_t> pose_ptr, pose_fac;
    // distinct neighbours of a pose, ascending, with the pair that joins them
    std::vector<int32_t> adj_ptr, adj_nbr, adj_pair;
    std::vector<int32_t> jl, jidx;         // junction -> pose (ascending); pose -> junction or -1
    // segments: interior slots seg_ptr[s] .. seg_ptr[s + 1], end junctions, and per slot the pose and the block
    // (row = this pose, column = the next pose, or junction b after the last) as pair * 2 + transposed
    std::vector<int32_t> seg_ptr, seg_a, seg_b, seg_first, slot_pose, slot_link, pose_slot;
    std::vector<int32_t> jj_pair;          // pairs that join two junctions directly
    // blocks (row junction >= column junction) that segments contribute to, sorted, with the contributions of a block in
    // segment order as seg * 4 + kind
    std::vector<int32_t> tgt_r, tgt_c, tgt_ptr, tgt_ent;
    int64_t n_cut = 0;                     // poses promoted by the PGO_SEG_MAX rule
    int64_t J() const { return (int64_t)jl.size(); }
    int64_t S() const { return (int64_t)seg_a.size(); }
    int64_t M() const { return (int64_t)slot_pose.size(); }
    int64_t P() const { return (int64_t)pa.size(); }
};

// block (row u, column v) of the pair that joins u and v, as pair * 2 + transposed; -1 when they are not neighbours
static inline int32_t pgo_plan_link(const PgoPlan &p, int32_t u, int32_t v) {
    for (int32_t k = p.adj_ptr[u]; k < p.adj_ptr[u + 1]; ++k)
        if (p.adj_nbr[k] == v) return p.adj_pair[k] * 2 + (u < v ? 0 : 1);
    return -1;
}

// walks every segment of the junction set `isj`; with `out` the segments are appended to the plan, otherwise only `seen` is set
static inline void pgo_plan_walk(PgoPlan &p, const std::vector<char> &isj, std::vector<char> &seen, bool out,
                                 std::vector<std::vector<int32_t>> *paths) {
    for (int64_t a = 0; a < p.n; ++a) {
        if (!isj[a]) continue;
        for (int32_t k = p.adj_ptr[a]; k < p.adj_ptr[a + 1]; ++k) {
            int32_t cur = p.adj_nbr[k], prev = (int32_t)a;
            if (isj[cur] || seen[cur]) continue;
            std::vector<int32_t> path;
            while (!isj[cur]) {
                seen[cur] = 1;
                path.push_back(cur);
                // a non-junction pose has exactly two distinct neighbours
                const int32_t q = p.adj_ptr[cur];
                const int32_t nxt = p.adj_nbr[q] == prev ? p.adj_nbr[q + 1] : p.adj_nbr[q];
                prev = cur;
                cur = nxt;
            }
            if (paths) paths->push_back(path);
            if (out) {
                p.seg_a.push_back(p.jidx[a]);
                p.seg_b.push_back(p.jidx[cur]);
                p.seg_first.push_back(pgo_plan_link(p, path[0], (int32_t)a));
                for (size_t s = 0; s < path.size(); ++s) {
                    p.pose_slot[path[s]] = (int32_t)p.slot_pose.size();
                    p.slot_pose.push_back(path[s]);
                    p.slot_link.push_back(pgo_plan_link(p, path[s], s + 1 < path.size() ? path[s + 1] : cur));
                }
                p.seg_ptr.push_back((int32_t)p.slot_pose.size());
            }
        }
    }
}

// n poses, nf edges (ei[k], ej[k]), the prior on pose `prior`.  Returns 0 or PGO_PLAN_E_*.
static inline int pgo_make_plan(int64_t n, int64_t nf, const int32_t *ei, const int32_t *ej, int64_t prior, PgoPlan *plan) {
    PgoPlan &p = *plan;
    p = PgoPlan();
    if (n < 1 || n > 0x3fffffff || nf < 0 || nf > 0x1fffffff || prior < 0 || prior >= n) return PGO_PLAN_E_ARG;
    for (int64_t k = 0; k < nf; ++k)
        if (ei[k] < 0 || ei[k] >= n || ej[k] < 0 || ej[k] >= n || ei[k] == ej[k]) return PGO_PLAN_E_ARG;
    p.n = n; p.nf = nf; p.prior = (int32_t)prior;

    // factors per pose (ascending factor index; the prior is factor nf, the last)
    p.pose_ptr.assign(n + 1, 0);
    for (int64_t k = 0; k < nf; ++k) { ++p.pose_ptr[ei[k] + 1]; ++p.pose_ptr[ej[k] + 1]; }
    ++p.pose_ptr[prior + 1];
    for (int64_t v = 0; v < n; ++v) p.pose_ptr[v + 1] += p.pose_ptr[v];
    p.pose_fac.assign(p.pose_ptr[n], 0);
    {
        std::vector<int32_t> at(p.pose_ptr.begin(), p.pose_ptr.end() - 1);
        for (int64_t k = 0; k < nf; ++k) {
            p.pose_fac[at[ei[k]]++] = (int32_t)(k * 4);
            p.pose_fac[at[ej[k]]++] = (int32_t)(k * 4 + 1);
        }
        p.pose_fac[at[prior]++] = (int32_t)(nf * 4 + 2);
    }

    // unique pairs, sorted by (min, max); the factors of a pair keep their order (stable sort)
    std::vector<int32_t> order(nf);
    for (int64_t k = 0; k < nf; ++k) order[k] = (int32_t)k;
    auto lo = [&](int32_t k) { return std::min(ei[k], ej[k]); };
    auto hi = [&](int32_t k) { return std::max(ei[k], ej[k]); };
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return lo(x) != lo(y) ? lo(x) < lo(y) : hi(x) < hi(y);
    });
    p.pair_ptr.push_back(0);
    for (int64_t q = 0; q < nf; ++q) {
        const int32_t k = order[q];
        if (q == 0 || lo(k) != p.pa.back() || hi(k) != p.pb.back()) {
            if (q) p.pair_ptr.push_back((int32_t)p.pair_fac.size());
            p.pa.push_back(lo(k));
            p.pb.push_back(hi(k));
        }
        p.pair_fac.push_back(k * 2 + (ei[k] > ej[k] ? 1 : 0));
    }
    if (nf) p.pair_ptr.push_back((int32_t)p.pair_fac.size());
    const int64_t P = p.P();

    // adjacency: pairs are sorted by (pa, pb), so filling in pair order leaves every list ascending
    p.adj_ptr.assign(n + 1, 0);
    for (int64_t q = 0; q < P; ++q) { ++p.adj_ptr[p.pa[q] + 1]; ++p.adj_ptr[p.pb[q] + 1]; }
    for (int64_t v = 0; v < n; ++v) p.adj_ptr[v + 1] += p.adj_ptr[v];
    p.adj_nbr.assign(p.adj_ptr[n], 0);
    p.adj_pair.assign(p.adj_ptr[n], 0);
    {
        std::vector<int32_t> at(p.adj_ptr.begin(), p.adj_ptr.end() - 1);
        // the lower neighbours of v (pairs with pb == v) come first in ascending pa, then the higher ones in ascending pb
        for (int64_t q = 0; q < P; ++q) { const int32_t v = p.pb[q]; p.adj_nbr[at[v]] = p.pa[q]; p.adj_pair[at[v]++] = (int32_t)q; }
        for (int64_t q = 0; q < P; ++q) { const int32_t v = p.pa[q]; p.adj_nbr[at[v]] = p.pb[q]; p.adj_pair[at[v]++] = (int32_t)q; }
    }

    // junctions: the prior, every pose without exactly two distinct neighbours, one pose of every junction-free cycle,
    // and the cuts of long interiors
    std::vector<char> isj(n, 0), seen(n, 0);
    for (int64_t v = 0; v < n; ++v) isj[v] = (p.adj_ptr[v + 1] - p.adj_ptr[v] != 2) || v == prior;
    p.jidx.assign(n, -1);                                       // pgo_plan_walk reads it only when it writes segments
    pgo_plan_walk(p, isj, seen, false, nullptr);
    for (int64_t v = 0; v < n; ++v) {
        if (isj[v] || seen[v]) continue;
        isj[v] = 1;                                             // the lowest pose of a cycle that has no junction
        pgo_plan_walk(p, isj, seen, false, nullptr);            // marks the rest of that cycle
    }
    {
        std::vector<std::vector<int32_t>> paths;
        std::fill(seen.begin(), seen.end(), 0);
        pgo_plan_walk(p, isj, seen, false, &paths);
        for (const std::vector<int32_t> &path : paths)
            if ((int64_t)path.size() > PGO_SEG_MAX)
                for (size_t s = PGO_SEG_MAX; s < path.size(); s += PGO_SEG_MAX + 1) { isj[path[s]] = 1; ++p.n_cut; }
    }
    for (int64_t v = 0; v < n; ++v)
        if (isj[v]) { p.jidx[v] = (int32_t)p.jl.size(); p.jl.push_back((int32_t)v); }
    if (p.J() > PGO_MAX_JUNCTIONS) return PGO_PLAN_E_LIMIT;

    // segments of the final junction set
    p.pose_slot.assign(n, -1);
    p.seg_ptr.push_back(0);
    std::fill(seen.begin(), seen.end(), 0);
    pgo_plan_walk(p, isj, seen, true, nullptr);
    for (int64_t q = 0; q < P; ++q)
        if (isj[p.pa[q]] && isj[p.pb[q]]) p.jj_pair.push_back((int32_t)q);

    // the blocks of the junction system that segments add into
    struct Ent { int32_t r, c, e; };
    std::vector<Ent> ents;
    for (int64_t s = 0; s < p.S(); ++s) {
        const int32_t a = p.seg_a[s], b = p.seg_b[s], s4 = (int32_t)(s * 4);
        ents.push_back(Ent{a, a, s4 + PGO_KIND_AA});
        ents.push_back(Ent{b, b, s4 + PGO_KIND_BB});
        if (a == b) { ents.push_back(Ent{a, a, s4 + PGO_KIND_AB}); ents.push_back(Ent{a, a, s4 + PGO_KIND_BA}); }
        else if (a > b) ents.push_back(Ent{a, b, s4 + PGO_KIND_AB});
        else ents.push_back(Ent{b, a, s4 + PGO_KIND_BA});
    }
    std::stable_sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.r != y.r ? x.r < y.r : x.c < y.c; });
    p.tgt_ptr.push_back(0);
    for (size_t q = 0; q < ents.size(); ++q) {
        if (q == 0 || ents[q].r != p.tgt_r.back() || ents[q].c != p.tgt_c.back()) {
            if (q) p.tgt_ptr.push_back((int32_t)p.tgt_ent.size());
            p.tgt_r.push_back(ents[q].r);
            p.tgt_c.push_back(ents[q].c);
        }
        p.tgt_ent.push_back(ents[q].e);
    }
    if (!ents.empty()) p.tgt_ptr.push_back((int32_t)p.tgt_ent.size());
    return 0;
}
