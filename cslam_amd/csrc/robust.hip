// robust.hip -- the robust coarse fit of a lidar loop closure from its mutual feature matches (gfx950).
//
// Replaces the TEASER++ step of `solve_teaser` (cslam/lidar_pr/icp_utils.py:68-83 `get_teaser_solver`, :116-121 the solve)
// for a batch of pairs: cbar2 = 1, no scale estimation, exact maximum clique, CHAIN graph for the rotation, GNC-TLS with
// factor 1.4 / 10000 iterations / cost threshold 1e-16, per-axis TLS for the translation.  The rules are spelled out in
// include/cslam_hip.h.  All arithmetic is float64 and nothing in this file is contracted: an fma is an fma only where it is
// written.  The one exception is the 4 x 4 eigen-solve of horn.h, included ahead of the pragma on purpose so that it is the
// same code as in icp.hip (the compiler's default contraction): deterministic all the same, a function of its 9 sums only.
//
//   rb_gather_kernel      : correspondence rows (i, j) -> the matched points, so that every stage reads two [N, 3] arrays.
//   rb_graph_kernel       : one wave per 64 rows of the consistency graph; the matched points go through LDS in chunks of
//                           RB_GRAPH_CHUNK; a lane owns its row's 64-bit word of 64 columns at a time.  Nothing is stored per
//                           pair of matches: the output is the N x N bit matrix and the degrees.
//   rb_prep_kernel        : one workgroup per pair: core numbers by peeling in rounds (degrees in LDS, integer atomics), the
//                           order (core number, index), and the greedy clique that is the lower bound of the search.
//   rb_permute_kernel     : the bit matrix relabelled by that order: a root's candidates are the bits above it.
//   rb_search_kernel      : one wave per root vertex, roots handed out from the top of the order by an integer atomic.  A
//                           set is a bitset spread over the lanes (two words each); branch and bound with a greedy colouring:
//                           only the vertices whose colour exceeds (bound - size so far) are branched on.  A root's search
//                           reads nothing another root writes, so what it finds does not depend on timing; the shared bound
//                           only skips whole roots that cannot hold a maximum clique.
//   rb_clique_final_kernel: the winner (largest, then the lowest root; the greedy clique unless a larger one exists) in
//                           ascending original indices.
//   rb_rotation_kernel    : one workgroup per pair loops GNC-TLS on the device: weighted Horn fit without centring (horn.h),
//                           residuals, weights; sums per thread in ascending k, then one fixed tree.
//   rb_translation_kernel : one workgroup per (pair, axis): the 2K interval endpoints ranked by counting on (value, index),
//                           a thread per interval centre, consensus sums in index order.
//   rb_assemble_kernel    : the 4 x 4 and the status of the chained call.
// No float atomics and no floating sum whose order depends on scheduling: a pair's bytes are the same alone or in any batch.
#include "common.h"
#include "horn.h"

#pragma clang fp contract(off)

#define ROBUST_MAX_N 8192          // most correspondences of a pair; above it the pair is not attempted (status 2)
#define RB_GRAPH_BLOCK 64          // rows of the graph per workgroup: one wave
#define RB_GRAPH_CHUNK 256         // matched points per LDS chunk of the graph kernel: 12 KiB; a multiple of 64
#define RB_BLOCK 256               // threads per workgroup of the other kernels
#define RB_STACK_DEPTH 512         // deepest branch of the clique search below a root; deeper ends the search uncertified
#define RB_MAX_WORDS (ROBUST_MAX_N / 64)
#define RB_GNC_MAX_ITER 10000
#define RB_GNC_FACTOR 1.4
#define RB_GNC_COST_TOL 1e-16
#define RB_FLAG_BUDGET 1
#define RB_FLAG_DEPTH 2

typedef unsigned long long u64;

struct RbState {                   // per pair, shared by the waves of the search
    int g;                         // size of the greedy clique
    int lb;                        // largest clique any root has found (>= g)
    int next_root;
    int flags;
    u64 nodes;
    u64 key;                       // (size << 32) | (n - root) of the best clique larger than the greedy one; 0 = none
};

// correspondences of pair p that are used: its count cut to its capacity; 0 when above the cap
__device__ __forceinline__ int rb_n(const int64_t *__restrict__ off, const int32_t *__restrict__ count, int p) {
    const int64_t cap = off[p + 1] - off[p];
    int64_t n = count ? (int64_t)count[p] : cap;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    return n > ROBUST_MAX_N ? 0 : (int)n;
}

__global__ __launch_bounds__(RB_BLOCK) void rb_gather_kernel(const double *__restrict__ src, const int64_t *__restrict__ src_off,
                                                            const double *__restrict__ dst, const int64_t *__restrict__ dst_off,
                                                            const int32_t *__restrict__ rows, const int64_t *__restrict__ off,
                                                            const int32_t *__restrict__ count, double *__restrict__ ms,
                                                            double *__restrict__ md) {
    const int p = blockIdx.y, n = rb_n(off, count, p);
    const int k = blockIdx.x * RB_BLOCK + threadIdx.x;
    if (k >= n) return;
    const int64_t base = off[p], ns = src_off[p + 1] - src_off[p], nd = dst_off[p + 1] - dst_off[p];
    const int64_t i = rows[2 * (base + k)], j = rows[2 * (base + k) + 1];
    const bool ok = i >= 0 && i < ns && j >= 0 && j < nd;      // a row that points outside its clouds matches nothing
    for (int a = 0; a < 3; ++a) {
        ms[3 * (base + k) + a] = ok ? src[3 * (src_off[p] + i) + a] : NAN;
        md[3 * (base + k) + a] = ok ? dst[3 * (dst_off[p] + j) + a] : NAN;
    }
}

// word offsets of the pairs' bit matrices: N rows of ceil(N / 64) words each
__global__ void rb_adj_off_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ count, int n_pairs,
                                  int64_t *__restrict__ adj_off) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t at = 0;
    for (int p = 0; p < n_pairs; ++p) {
        adj_off[p] = at;
        const int64_t n = rb_n(off, count, p);
        at += n * ((n + 63) >> 6);
    }
    adj_off[n_pairs] = at;
}

__global__ __launch_bounds__(RB_GRAPH_BLOCK) void rb_graph_kernel(const double *__restrict__ ms, const double *__restrict__ md,
                                                                 const int64_t *__restrict__ off, const int32_t *__restrict__ count,
                                                                 double two_c, u64 *__restrict__ adj,
                                                                 const int64_t *__restrict__ adj_off, int32_t *__restrict__ deg) {
    __shared__ double s_p[6 * RB_GRAPH_CHUNK];             // source rows, then target rows
    const int p = blockIdx.y, t = threadIdx.x, n = rb_n(off, count, p);
    const int i0 = blockIdx.x * RB_GRAPH_BLOCK;
    if (i0 >= n) return;                                   // the whole workgroup leaves
    const int W = (n + 63) >> 6, i = i0 + t;
    const bool live = i < n;
    const int64_t base = off[p];
    double sx = 0.0, sy = 0.0, sz = 0.0, tx = 0.0, ty = 0.0, tz = 0.0;
    if (live) {
        sx = ms[3 * (base + i)]; sy = ms[3 * (base + i) + 1]; sz = ms[3 * (base + i) + 2];
        tx = md[3 * (base + i)]; ty = md[3 * (base + i) + 1]; tz = md[3 * (base + i) + 2];
    }
    u64 *row = adj + adj_off[p] + (int64_t)i * W;
    int d = 0;
    for (int c0 = 0; c0 < n; c0 += RB_GRAPH_CHUNK) {
        const int cm = n - c0 < RB_GRAPH_CHUNK ? n - c0 : RB_GRAPH_CHUNK;
        __syncthreads();                                   // the previous chunk has been consumed
        for (int e = t; e < 3 * cm; e += RB_GRAPH_BLOCK) {
            s_p[e] = ms[3 * (base + c0) + e];
            s_p[3 * RB_GRAPH_CHUNK + e] = md[3 * (base + c0) + e];
        }
        __syncthreads();
        if (!live) continue;
        for (int w0 = 0; w0 < cm; w0 += 64) {
            const int lim = cm - w0 < 64 ? cm - w0 : 64;
            u64 word = 0;
            for (int b = 0; b < lim; ++b) {                // every lane reads the same point: a broadcast
                const double *q = s_p + 3 * (w0 + b), *r = q + 3 * RB_GRAPH_CHUNK;
                double dx = q[0] - sx, dy = q[1] - sy, dz = q[2] - sz;
                const double la = sqrt(fma(dz, dz, fma(dy, dy, __dmul_rn(dx, dx))));
                dx = r[0] - tx; dy = r[1] - ty; dz = r[2] - tz;
                const double lb = sqrt(fma(dz, dz, fma(dy, dy, __dmul_rn(dx, dx))));
                const bool edge = fabs(lb - la) <= two_c && c0 + w0 + b != i;
                word |= (u64)(edge ? 1 : 0) << b;
            }
            row[(c0 + w0) >> 6] = word;
            d += (int)__popcll(word);
        }
    }
    if (live) deg[base + i] = d;
}

// ---- maximum clique ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB_BLOCK) void rb_prep_kernel(const u64 *__restrict__ adj, const int64_t *__restrict__ adj_off,
                                                          const int32_t *__restrict__ deg, const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ count, int32_t *__restrict__ core_sorted,
                                                          int32_t *__restrict__ ord, int32_t *__restrict__ greedy,
                                                          RbState *__restrict__ state) {
    __shared__ int s_deg[ROBUST_MAX_N];                    // 32 KiB
    __shared__ short s_core[ROBUST_MAX_N];                 // 16 KiB; -1 = not peeled yet
    __shared__ u64 s_P[RB_MAX_WORDS];
    __shared__ int s_min, s_cnt, s_key;
    const int p = blockIdx.x, t = threadIdx.x, n = rb_n(off, count, p);
    if (t == 0) {
        state[p].g = 0; state[p].lb = 0; state[p].next_root = 0; state[p].flags = 0; state[p].nodes = 0; state[p].key = 0;
    }
    if (n <= 0) return;
    const int W = (n + 63) >> 6;
    const int64_t base = off[p];
    const u64 *A = adj + adj_off[p];
    int32_t *frontier = ord + base;                        // the order is written after the peeling
    for (int v = t; v < n; v += RB_BLOCK) { s_deg[v] = deg[base + v]; s_core[v] = -1; }
    __syncthreads();
    // core numbers: at level k, vertices of remaining degree <= k are peeled round by round until none is left
    while (true) {
        if (t == 0) s_min = 0x7fffffff;
        __syncthreads();
        int lm = 0x7fffffff;
        for (int v = t; v < n; v += RB_BLOCK)
            if (s_core[v] < 0 && s_deg[v] < lm) lm = s_deg[v];
        if (lm != 0x7fffffff) atomicMin(&s_min, lm);
        __syncthreads();
        const int k = s_min;
        if (k == 0x7fffffff) break;
        while (true) {
            __syncthreads();                               // s_cnt of the previous round has been read
            if (t == 0) s_cnt = 0;
            __syncthreads();
            for (int v = t; v < n; v += RB_BLOCK)
                if (s_core[v] < 0 && s_deg[v] <= k) {
                    s_core[v] = (short)k;
                    frontier[atomicAdd(&s_cnt, 1)] = v;
                }
            __threadfence_block();
            __syncthreads();
            const int cnt = s_cnt;
            if (cnt == 0) break;
            for (int e = t; e < cnt * W; e += RB_BLOCK) {
                const int v = frontier[e / W], w = e % W;
                u64 word = A[(int64_t)v * W + w];
                while (word) {
                    const int b = __ffsll(word) - 1;
                    word &= word - 1;
                    atomicSub(&s_deg[w * 64 + b], 1);
                }
            }
        }
    }
    __syncthreads();
    // the order of the search: ascending (core number, index), by counting
    for (int v = t; v < n; v += RB_BLOCK) {
        const int cv = s_core[v];
        int r = 0;
        for (int u = 0; u < n; ++u) {
            const int cu = s_core[u];
            r += (cu < cv || (cu == cv && u < v)) ? 1 : 0;
        }
        ord[base + r] = v;
        core_sorted[base + r] = cv;
    }
    // the greedy clique: the vertex of largest core number (the lowest index of equals), then again and again the same
    // choice among the common neighbours of those taken
    for (int w = t; w < W; w += RB_BLOCK) {
        const int left = n - 64 * w;
        s_P[w] = left >= 64 ? ~0ull : ((1ull << left) - 1);
    }
    int g = 0;
    while (true) {
        __syncthreads();
        if (t == 0) s_key = -1;
        __syncthreads();
        int best = -1;
        for (int v = t; v < n; v += RB_BLOCK)
            if ((s_P[v >> 6] >> (v & 63)) & 1ull) {
                const int key = ((int)s_core[v] << 13) | (ROBUST_MAX_N - 1 - v);
                best = key > best ? key : best;
            }
        if (best >= 0) atomicMax(&s_key, best);
        __syncthreads();
        if (s_key < 0) break;
        const int u = ROBUST_MAX_N - 1 - (s_key & (ROBUST_MAX_N - 1));
        if (t == 0) greedy[base + g] = u;
        ++g;
        for (int w = t; w < W; w += RB_BLOCK)               // never u itself, whatever the diagonal of a given matrix holds
            s_P[w] &= A[(int64_t)u * W + w] & ~(w == (u >> 6) ? 1ull << (u & 63) : 0ull);
    }
    if (t == 0) { state[p].g = g; state[p].lb = g; }
}

__global__ __launch_bounds__(RB_BLOCK) void rb_permute_kernel(const u64 *__restrict__ adj, const int64_t *__restrict__ adj_off,
                                                             const int64_t *__restrict__ off, const int32_t *__restrict__ count,
                                                             const int32_t *__restrict__ ord, u64 *__restrict__ adjp) {
    const int p = blockIdx.y, n = rb_n(off, count, p);
    const int W = (n + 63) >> 6;
    const int64_t e = (int64_t)blockIdx.x * RB_BLOCK + threadIdx.x;
    if (e >= (int64_t)n * W) return;
    const int i = (int)(e / W), wj = (int)(e % W);
    const int32_t *o = ord + off[p];
    const u64 *row = adj + adj_off[p] + (int64_t)o[i] * W;
    const int lim = n - 64 * wj < 64 ? n - 64 * wj : 64;
    u64 word = 0;
    for (int b = 0; b < lim; ++b) {
        const int u = o[64 * wj + b];
        word |= ((row[u >> 6] >> (u & 63)) & 1ull) << b;
    }
    adjp[adj_off[p] + e] = word;
}

// the lowest member of a set spread over the wave (lane l holds words l and l + 64), -1 for the empty set; wave-uniform
__device__ __forceinline__ int rb_first(u64 c0, u64 c1, int lane) {
    u64 m = __ballot(c0 != 0);
    int hi = 0;
    if (!m) {
        m = __ballot(c1 != 0);
        if (!m) return -1;
        hi = 1;
    }
    const int l = __ffsll(m) - 1;
    const u64 w = __shfl(hi ? c1 : c0, l, 64);
    return (hi * 64 + l) * 64 + __ffsll(w) - 1;
}

// Greedy colouring of P in index order, class by class; (b0, b1) = the members whose colour exceeds kmin.  A clique inside
// the others has at most kmin members, so a clique of more than kmin members of P holds one of (b0, b1).
__device__ __forceinline__ void rb_colour(const u64 *__restrict__ A, int W, int lane, u64 p0, u64 p1, int kmin, u64 *b0, u64 *b1) {
    if (kmin <= 0) { *b0 = p0; *b1 = p1; return; }
    u64 q0 = p0, q1 = p1, r0 = 0, r1 = 0;
    int k = 0;
    while (__ballot((q0 | q1) != 0)) {
        ++k;
        u64 c0 = q0, c1 = q1;
        while (true) {
            const int v = rb_first(c0, c1, lane);
            if (v < 0) break;
            const int w = v >> 6;
            const u64 bit = 1ull << (v & 63);
            const u64 a0 = lane < W ? A[(int64_t)v * W + lane] : 0ull;
            const u64 a1 = lane + 64 < W ? A[(int64_t)v * W + lane + 64] : 0ull;
            c0 &= ~a0; c1 &= ~a1;
            if (w == lane) { c0 &= ~bit; q0 &= ~bit; if (k > kmin) r0 |= bit; }
            if (w == lane + 64) { c1 &= ~bit; q1 &= ~bit; if (k > kmin) r1 |= bit; }
        }
    }
    *b0 = r0; *b1 = r1;
}

// a level of a wave's stack: P and B, `halves` words per lane for the first `wl` lanes (the others hold no word of the widest pair)
#define RB_STK(d, s, h) stk[(((int64_t)(d) * 2 + (s)) * halves + (h)) * wl + lane]
#define RB_STK_SAVE(d)                                                              \
    if (lane < wl) {                                                                \
        RB_STK(d, 0, 0) = p0; RB_STK(d, 1, 0) = b0;                                 \
        if (halves == 2) { RB_STK(d, 0, 1) = p1; RB_STK(d, 1, 1) = b1; }            \
    }
#define RB_STK_LOAD(d)                                                              \
    p0 = p1 = b0 = b1 = 0;                                                          \
    if (lane < wl) {                                                                \
        p0 = RB_STK(d, 0, 0); b0 = RB_STK(d, 1, 0);                                 \
        if (halves == 2) { p1 = RB_STK(d, 0, 1); b1 = RB_STK(d, 1, 1); }            \
    }

__global__ __launch_bounds__(64) void rb_search_kernel(const u64 *__restrict__ adjp, const int64_t *__restrict__ adj_off,
                                                      const int32_t *__restrict__ core_sorted, const int64_t *__restrict__ off,
                                                      const int32_t *__restrict__ count, RbState *__restrict__ state, u64 budget,
                                                      u64 *__restrict__ stack, int64_t stack_words, int wl, int halves,
                                                      int32_t *__restrict__ wbest,
                                                      u64 *__restrict__ wkey) {
    __shared__ int s_R[RB_STACK_DEPTH + 1];
    const int p = blockIdx.y, lane = threadIdx.x, n = rb_n(off, count, p);
    const int64_t wave = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    u64 mykey = 0;
    if (n > 0) {
        const int W = (n + 63) >> 6;
        const int64_t base = off[p];
        const u64 *A = adjp + adj_off[p];
        RbState *S = state + p;
        u64 *stk = stack + wave * stack_words;             // [depth][P | B][halves][wl]
        int32_t *mybest = wbest + wave * (RB_STACK_DEPTH + 1);
        const int g = S->g;
        bool stop = false;
        while (!stop) {
            int r = 0;
            if (lane == 0) r = atomicAdd(&S->next_root, 1);
            r = __shfl(r, 0, 64);
            if (r >= n) break;
            const int root = n - 1 - r;
            const int ub = core_sorted[base + root] + 1;   // a clique of `root` and later vertices has at most this many
            if (ub <= g) break;                            // and so have all roots below it
            int lb = 0, fl = 0;
            if (lane == 0) { lb = atomicAdd(&S->lb, 0); fl = atomicAdd(&S->flags, 0); }
            lb = __shfl(lb, 0, 64); fl = __shfl(fl, 0, 64);
            if (fl) break;
            if (ub < lb) continue;                         // strictly: a root that may hold a clique of the largest size is searched
            int own = g, d = 0;
            u64 p0 = lane < W ? A[(int64_t)root * W + lane] : 0ull;
            u64 p1 = lane + 64 < W ? A[(int64_t)root * W + lane + 64] : 0ull;
            {                                              // the candidates of a root are its neighbours above it
                const int rw = root >> 6;
                const u64 above = (root & 63) == 63 ? 0ull : ~0ull << ((root & 63) + 1);
                if (lane < rw) p0 = 0; else if (lane == rw) p0 &= above;
                if (lane + 64 < rw) p1 = 0; else if (lane + 64 == rw) p1 &= above;
            }
            if (lane == 0) s_R[0] = root;
            bool enter = true;
            u64 b0 = 0, b1 = 0;
            while (true) {
                if (enter) {                               // a node: R = s_R[0 .. d], P = (p0, p1)
                    u64 cnt = 0;
                    if (lane == 0) cnt = atomicAdd(&S->nodes, 1ull);
                    cnt = __shfl(cnt, 0, 64);
                    if (cnt >= budget) {
                        if (lane == 0) atomicOr(&S->flags, RB_FLAG_BUDGET);
                        stop = true;
                        break;
                    }
                    if (!__ballot((p0 | p1) != 0)) {
                        b0 = b1 = 0;
                        if (d + 1 > own) {                 // a larger clique than this root had
                            own = d + 1;
                            const u64 key = ((u64)own << 32) | (u64)(n - root);
                            if (key > mykey) {
                                mykey = key;
                                __builtin_amdgcn_wave_barrier();
                                for (int e = lane; e <= d; e += 64) mybest[e] = s_R[e];
                            }
                        }
                    } else {
                        rb_colour(A, W, lane, p0, p1, own - (d + 1), &b0, &b1);
                    }
                    RB_STK_SAVE(d);
                    enter = false;
                }
                const int v = rb_first(b0, b1, lane);
                if (v < 0) {                               // nothing left to branch on: back to the parent
                    if (--d < 0) break;
                    RB_STK_LOAD(d);
                    continue;
                }
                const int w = v >> 6;
                const u64 bit = 1ull << (v & 63);
                if (w == lane) { p0 &= ~bit; b0 &= ~bit; }
                if (w == lane + 64) { p1 &= ~bit; b1 &= ~bit; }
                if (d + 1 >= RB_STACK_DEPTH) {
                    if (lane == 0) atomicOr(&S->flags, RB_FLAG_DEPTH);
                    stop = true;
                    break;
                }
                RB_STK_SAVE(d);
                p0 &= lane < W ? A[(int64_t)v * W + lane] : 0ull;
                p1 &= lane + 64 < W ? A[(int64_t)v * W + lane + 64] : 0ull;
                ++d;
                if (lane == 0) s_R[d] = v;
                __builtin_amdgcn_wave_barrier();
                enter = true;
            }
            if (own > g && lane == 0) {
                atomicMax(&S->lb, own);
                atomicMax(&S->key, ((u64)own << 32) | (u64)(n - root));
            }
        }
    }
    if (lane == 0) wkey[wave] = mykey;
}

__global__ __launch_bounds__(RB_BLOCK) void rb_clique_final_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ count,
                                                                  const int32_t *__restrict__ ord, const int32_t *__restrict__ greedy,
                                                                  const RbState *__restrict__ state, const int32_t *__restrict__ wbest,
                                                                  const u64 *__restrict__ wkey, int slots, int32_t *__restrict__ clique,
                                                                  int32_t *__restrict__ clique_size, int32_t *__restrict__ certified,
                                                                  int64_t *__restrict__ nodes) {
    __shared__ u64 s_set[RB_MAX_WORDS];
    __shared__ int s_wave;
    const int p = blockIdx.x, t = threadIdx.x, n = rb_n(off, count, p);
    const int64_t base = off[p];
    const RbState S = state[p];
    if (t == 0) {
        certified[p] = S.flags == 0 ? 1 : 0;
        if (nodes) nodes[p] = (int64_t)S.nodes;
        s_wave = -1;
    }
    const int W = (n + 63) >> 6;
    for (int w = t; w < RB_MAX_WORDS; w += RB_BLOCK) s_set[w] = 0;
    __syncthreads();
    int size = S.g;
    if (S.key) {
        for (int s = t; s < slots; s += RB_BLOCK)
            if (wkey[(int64_t)p * slots + s] == S.key) s_wave = s;      // one wave searched that root
        __syncthreads();
    }
    if (S.key && s_wave >= 0) {
        size = (int)(S.key >> 32);
        const int32_t *best = wbest + ((int64_t)p * slots + s_wave) * (RB_STACK_DEPTH + 1);
        for (int e = t; e < size; e += RB_BLOCK) {
            const int v = ord[base + best[e]];
            atomicOr(&s_set[v >> 6], 1ull << (v & 63));
        }
    } else {
        for (int e = t; e < size; e += RB_BLOCK) {
            const int v = greedy[base + e];
            atomicOr(&s_set[v >> 6], 1ull << (v & 63));
        }
    }
    __syncthreads();
    for (int w = t; w < W; w += RB_BLOCK) {                // ascending indices
        int at = 0;
        for (int x = 0; x < w; ++x) at += (int)__popcll(s_set[x]);
        u64 word = s_set[w];
        while (word) {
            clique[base + at++] = 64 * w + __ffsll(word) - 1;
            word &= word - 1;
        }
    }
    if (t == 0) clique_size[p] = size;
}

// ---- rotation ------------------------------------------------------------------------------------------------------
// fixed-order sum of NV values over the workgroup: lanes by one shuffle tree, waves in order; thread 0 holds the result
template <int NV>
__device__ __forceinline__ void rb_block_sum(double *v, double (*s_w)[10], int t) {
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double x = v[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) x += __shfl_down(x, o, 64);
        if ((t & 63) == 0) s_w[t >> 6][k] = x;
    }
    __syncthreads();
    if (t == 0)
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double a = s_w[0][k];
            for (int w = 1; w < RB_BLOCK / 64; ++w) a += s_w[w][k];
            v[k] = a;
        }
}

__device__ __forceinline__ void rb_tim(const double *__restrict__ ms, const double *__restrict__ md, const int32_t *__restrict__ q,
                                       int k, double *a, double *b) {
    const int64_t u = q[k], v = q[k + 1];
    for (int x = 0; x < 3; ++x) { a[x] = ms[3 * v + x] - ms[3 * u + x]; b[x] = md[3 * v + x] - md[3 * u + x]; }
}

__device__ __forceinline__ double rb_residual2(const double *R, const double *a, const double *b) {
    const double rx = b[0] - (R[0] * a[0] + R[1] * a[1] + R[2] * a[2]);
    const double ry = b[1] - (R[3] * a[0] + R[4] * a[1] + R[5] * a[2]);
    const double rz = b[2] - (R[6] * a[0] + R[7] * a[1] + R[8] * a[2]);
    return rx * rx + ry * ry + rz * rz;
}

__global__ __launch_bounds__(RB_BLOCK) void rb_rotation_kernel(const double *__restrict__ ms, const double *__restrict__ md,
                                                              const int64_t *__restrict__ off, const int32_t *__restrict__ clique,
                                                              const int32_t *__restrict__ clique_size, double nb2,
                                                              double *__restrict__ R_out, double *__restrict__ weights,
                                                              int32_t *__restrict__ iters_out) {
    __shared__ double s_w[RB_BLOCK / 64][10];
    __shared__ double s_R[9], s_ctl[3];
    __shared__ int s_stop;
    const int p = blockIdx.x, t = threadIdx.x;
    const int64_t base = off[p], cap = off[p + 1] - base;
    int K = clique_size[p];
    K = K > cap ? (int)cap : K;
    const int M = K - 1;
    if (M < 1) {
        if (t < 9) R_out[9 * (int64_t)p + t] = t % 4 == 0 ? 1.0 : 0.0;
        if (t == 0) iters_out[p] = 0;
        return;
    }
    const double *S = ms + 3 * base, *D = md + 3 * base;
    const int32_t *q = clique + base;
    double *w = weights + base;                            // a thread reads and writes its own entries only
    for (int k = t; k < M; k += RB_BLOCK) w[k] = 1.0;
    double mu = 1.0, prev = INFINITY;                      // thread 0's
    int iters = 0;
    for (int it = 0; it < RB_GNC_MAX_ITER; ++it) {
        double v[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) v[e] = 0.0;
        for (int k = t; k < M; k += RB_BLOCK) {
            double a[3], b[3];
            rb_tim(S, D, q, k, a, b);
            const double wk = w[k];
#pragma unroll
            for (int y = 0; y < 3; ++y)
#pragma unroll
                for (int x = 0; x < 3; ++x) v[3 * y + x] += wk * (b[y] * a[x]);
        }
        rb_block_sum<9>(v, s_w, t);
        if (t == 0) {                                      // argmax sum w b . (R a): Horn's form without centring
            double s[17], U[12];
            for (int e = 0; e < 17; ++e) s[e] = 0.0;
            s[0] = 1.0;
            for (int e = 0; e < 9; ++e) s[7 + e] = v[e];
            icp_rigid_from_sums(s, U);
            for (int y = 0; y < 3; ++y)
                for (int x = 0; x < 3; ++x) s_R[3 * y + x] = U[4 * y + x];
        }
        __syncthreads();
        double R[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) R[e] = s_R[e];
        double c[1] = {0.0}, mx = 0.0;
        for (int k = t; k < M; k += RB_BLOCK) {
            double a[3], b[3];
            rb_tim(S, D, q, k, a, b);
            const double r2 = rb_residual2(R, a, b);
            c[0] += w[k] * r2;
            mx = r2 > mx ? r2 : mx;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { const double y = __shfl_xor(mx, o, 64); mx = y > mx ? y : mx; }
        if ((t & 63) == 0) s_w[t >> 6][9] = mx;
        rb_block_sum<1>(c, s_w, t);
        if (t == 0) {
            int stop = 0;
            if (it == 0) {
                for (int x = 1; x < RB_BLOCK / 64; ++x) mx = s_w[x][9] > mx ? s_w[x][9] : mx;
                mu = 1.0 / (2.0 * mx / nb2 - 1.0);
                if (mu <= 0.0) stop = 1;                   // every residual is within the bound: the unit weights stand
            }
            if (!stop) {
                s_ctl[0] = (mu + 1.0) / mu * nb2;
                s_ctl[1] = mu / (mu + 1.0) * nb2;
                s_ctl[2] = mu;
                const double d = fabs(c[0] - prev);
                mu *= RB_GNC_FACTOR;
                prev = c[0];
                if (d < RB_GNC_COST_TOL) stop = 2;         // after this round's weights
            }
            s_stop = stop;
        }
        __syncthreads();
        const int stop = s_stop;
        if (stop == 1) break;
        const double th1 = s_ctl[0], th2 = s_ctl[1], m = s_ctl[2];
        for (int k = t; k < M; k += RB_BLOCK) {
            double a[3], b[3];
            rb_tim(S, D, q, k, a, b);
            const double r2 = rb_residual2(R, a, b);
            w[k] = r2 >= th1 ? 0.0 : (r2 <= th2 ? 1.0 : sqrt(nb2 * m * (m + 1.0) / r2) - m);
        }
        iters = it + 1;
        if (stop == 2) break;
        __syncthreads();                                   // s_stop and s_ctl have been read
    }
    if (t < 9) R_out[9 * (int64_t)p + t] = s_R[t];
    if (t == 0) iters_out[p] = iters;
}

// ---- translation ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RB_BLOCK) void rb_translation_kernel(const double *__restrict__ ms, const double *__restrict__ md,
                                                                 const int64_t *__restrict__ off, const int32_t *__restrict__ clique,
                                                                 const int32_t *__restrict__ clique_size, const double *__restrict__ Rs,
                                                                 double c, int64_t total, double *__restrict__ xs,
                                                                 double *__restrict__ sorted, double *__restrict__ t_out,
                                                                 int32_t *__restrict__ set_out) {
    __shared__ double s_cost[RB_BLOCK];
    __shared__ int s_m[RB_BLOCK];
    const int axis = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
    const int64_t base = off[p], cap = off[p + 1] - base;
    int K = clique_size[p];
    K = K > cap ? (int)cap : K;
    if (K < 1) {
        if (t == 0) t_out[3 * (int64_t)p + axis] = 0.0;
        return;
    }
    const double *R = Rs + 9 * (int64_t)p + 3 * axis;
    const int32_t *q = clique + base;
    double *x = xs + axis * total + base, *so = sorted + 2 * (axis * total + base);
    for (int k = t; k < K; k += RB_BLOCK) {
        const double *s = ms + 3 * (base + q[k]);
        x[k] = md[3 * (base + q[k]) + axis] - ((R[0] * s[0] + R[1] * s[1]) + R[2] * s[2]);
    }
    __threadfence_block();
    __syncthreads();
    for (int e = t; e < 2 * K; e += RB_BLOCK) {            // rank of endpoint e in the order (value, index)
        const double val = (e & 1) ? x[e >> 1] + c : x[e >> 1] - c;
        int r = 0;
        for (int o = 0; o < 2 * K; ++o) {
            const double vo = (o & 1) ? x[o >> 1] + c : x[o >> 1] - c;
            r += (vo < val || (vo == val && o < e)) ? 1 : 0;
        }
        so[r] = val;
    }
    __threadfence_block();
    __syncthreads();
    double best = INFINITY;
    int bm = -1;
    for (int m = t; m < 2 * K - 1; m += RB_BLOCK) {
        const double centre = (so[m] + so[m + 1]) * 0.5;
        double sum = 0.0;
        int cnt = 0;
        for (int k = 0; k < K; ++k)
            if (fabs(x[k] - centre) <= c) { sum += x[k]; ++cnt; }
        if (cnt == 0) continue;                            // a centre in a gap has no estimate
        const double est = sum / (double)cnt;
        double res = 0.0;
        for (int k = 0; k < K; ++k)
            if (fabs(x[k] - centre) <= c) { const double d = x[k] - est; res += d * d; }
        const double cost = res + c * (double)(K - cnt);
        if (cost < best) { best = cost; bm = m; }          // strict: the lower centre of equal costs stays
    }
    s_cost[t] = best;
    s_m[t] = bm;
    __syncthreads();
    if (t == 0) {
        for (int o = 1; o < RB_BLOCK; ++o)
            if (s_m[o] >= 0 && (s_m[0] < 0 || s_cost[o] < s_cost[0] || (s_cost[o] == s_cost[0] && s_m[o] < s_m[0]))) {
                s_cost[0] = s_cost[o];
                s_m[0] = s_m[o];
            }
    }
    __syncthreads();
    bm = s_m[0];
    double centre = 0.0, sum = 0.0;
    int cnt = 0;
    if (bm >= 0) {
        centre = (so[bm] + so[bm + 1]) * 0.5;
        for (int k = 0; k < K; ++k)
            if (fabs(x[k] - centre) <= c) { sum += x[k]; ++cnt; }
    }
    if (t == 0) t_out[3 * (int64_t)p + axis] = cnt > 0 ? sum / (double)cnt : 0.0;
    if (set_out)
        for (int k = t; k < K; k += RB_BLOCK) set_out[axis * total + base + k] = (bm >= 0 && fabs(x[k] - centre) <= c) ? 1 : 0;
}

__global__ void rb_assemble_kernel(const int64_t *__restrict__ off, const int32_t *__restrict__ count, int n_pairs,
                                   const int32_t *__restrict__ clique_size, const int32_t *__restrict__ certified,
                                   const int64_t *__restrict__ nodes, const double *__restrict__ R, const double *__restrict__ tr,
                                   const int32_t *__restrict__ iters, double *__restrict__ T, int64_t *__restrict__ info) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const int64_t cap = off[p + 1] - off[p];
    int64_t n = count ? (int64_t)count[p] : cap;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int K = clique_size[p];
    const int status = n > ROBUST_MAX_N ? 2 : (K < 3 ? 1 : 0);
    double *Tp = T + 16 * (int64_t)p;
    for (int e = 0; e < 16; ++e) Tp[e] = e % 5 == 0 ? 1.0 : 0.0;
    if (status == 0)
        for (int a = 0; a < 3; ++a) {
            for (int b = 0; b < 3; ++b) Tp[4 * a + b] = R[9 * (int64_t)p + 3 * a + b];
            Tp[4 * a + 3] = tr[3 * (int64_t)p + a];
        }
    int64_t *o = info + 6 * (int64_t)p;
    o[0] = status; o[1] = K; o[2] = status == 0 ? iters[p] : 0; o[3] = certified[p]; o[4] = nodes[p]; o[5] = n;
}

// ---- host side -------------------------------------------------------------------------------------------------------
static StreamScratch g_robust_scratch;

// the shared offsets rule and the one limit of this family
static int rb_shape(const int64_t *off, int n_pairs, RaggedShape *s) {
    int rc = offsets_check(off, n_pairs, s);
    if (rc) return rc;
    ARG_CHECK(s->total <= 0x7fffffffll / 8, "too many correspondence rows in one call");
    return CSLAM_OK;
}

// what the caller's host copies allow to check before anything touches HIP
static int rb_host_checks(const int64_t *h_off, const int32_t *h_count, int n_pairs) {
    if (!h_off) return CSLAM_OK;
    RaggedShape s;
    int rc = rb_shape(h_off, n_pairs, &s);
    if (rc) return rc;
    for (int p = 0; h_count && p < n_pairs; ++p)
        ARG_CHECK(h_count[p] >= 0 && h_count[p] <= h_off[p + 1] - h_off[p], "a count is negative or beyond its pair's rows");
    return CSLAM_OK;
}

struct RbPlan {
    std::vector<int32_t> cnt;                              // the counts that are used: cut to the capacity, 0 above the cap
    int64_t total = 0, adj_words = 0;
    int max_n = 0;
};

// Offsets and counts on the host: the caller's copies, or one read-back of both and the one host wait of such a call.
static int rb_plan(const int64_t *d_off, const int32_t *d_count, const int64_t *h_off, const int32_t *h_count, int n_pairs,
                   hipStream_t st, RbPlan *pl) {
    std::vector<int64_t> own;
    int rc;
    if (h_off && (h_count || !d_count)) {
        if (d_count) pl->cnt.assign(h_count, h_count + n_pairs);
    } else {
        if ((rc = read_back_async(own, d_off, (size_t)n_pairs + 1, st))) return rc;
        if (d_count && (rc = read_back_async(pl->cnt, d_count, (size_t)n_pairs, st))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        h_off = own.data();
    }
    RaggedShape s;
    if ((rc = rb_shape(h_off, n_pairs, &s))) return rc;
    pl->total = s.total;
    pl->cnt.resize((size_t)n_pairs);
    for (int p = 0; p < n_pairs; ++p) {
        const int64_t cap = h_off[p + 1] - h_off[p];
        int64_t n = d_count ? pl->cnt[p] : cap;
        n = n < 0 ? 0 : (n > cap ? cap : n);
        n = n > ROBUST_MAX_N ? 0 : n;
        pl->cnt[p] = (int32_t)n;
        pl->adj_words += n * ((n + 63) / 64);
        if (n > pl->max_n) pl->max_n = (int)n;
    }
    return CSLAM_OK;
}

#define RB_PLAN(pl, d_off, d_count, h_off, h_count, n_pairs, first_ptr)                                   \
    {                                                                                                     \
        int _rc = rb_host_checks((h_off), (d_count) ? (h_count) : nullptr, (n_pairs));                    \
        if (_rc) return _rc;                                                                              \
    }                                                                                                     \
    PTR_DEVICE(first_ptr);                                                                                \
    hipStream_t st = (hipStream_t)stream;                                                                 \
    RbPlan pl;                                                                                            \
    {                                                                                                     \
        int _rc = rb_plan((d_off), (d_count), (h_off), (h_count), (n_pairs), st, &pl);                    \
        if (_rc) return _rc;                                                                              \
    }

// a piece of this family's scratch: 8 bytes of slack behind each
template <typename T> static T *rb_take(Carver &cv, size_t n) { return cv.take<T>(n, 8); }

struct RbCliqueWs {
    int32_t *core_sorted, *ord, *greedy, *wbest;
    u64 *adjp, *stack, *wkey;
    RbState *state;
    int slots, wl, halves;
    int64_t stack_words;
};

static void rb_clique_carve(Carver &cv, const RbPlan &pl, int n_pairs, RbCliqueWs *ws) {
    const int max_w = (pl.max_n + 63) / 64;
    ws->wl = max_w < 64 ? (max_w > 0 ? max_w : 1) : 64;
    ws->halves = max_w > 64 ? 2 : 1;
    const int depth = pl.max_n < RB_STACK_DEPTH ? pl.max_n + 1 : RB_STACK_DEPTH;
    ws->stack_words = (int64_t)depth * 2 * ws->halves * ws->wl;
    int cu = cslam_cu_count();
    cu = cu > 0 ? cu : 256;
    int64_t slots = (int64_t)2 * cu / n_pairs;             // about two waves per compute unit in all ...
    const int64_t fit = ((int64_t)256 << 20) / (ws->stack_words * 8 * n_pairs);     // ... and 256 MiB of stacks at most
    slots = slots > fit ? fit : slots;
    slots = slots < 1 ? 1 : (slots > 256 ? 256 : slots);   // a large batch of large pairs runs with one wave per pair
    slots = slots > pl.max_n ? (pl.max_n > 0 ? pl.max_n : 1) : slots;
    ws->slots = (int)slots;
    const size_t waves = (size_t)slots * n_pairs;
    ws->core_sorted = rb_take<int32_t>(cv, (size_t)pl.total);
    ws->ord = rb_take<int32_t>(cv, (size_t)pl.total);
    ws->greedy = rb_take<int32_t>(cv, (size_t)pl.total);
    ws->adjp = rb_take<u64>(cv, (size_t)pl.adj_words);
    ws->state = rb_take<RbState>(cv, (size_t)n_pairs);
    ws->stack = rb_take<u64>(cv, waves * (size_t)ws->stack_words);
    ws->wbest = rb_take<int32_t>(cv, waves * (RB_STACK_DEPTH + 1));
    ws->wkey = rb_take<u64>(cv, waves);
}

static void rb_launch_graph(const double *ms, const double *md, const int64_t *d_off, const int32_t *d_count, int n_pairs,
                            const RbPlan &pl, double c, u64 *adj, int64_t *adj_off, int32_t *deg, hipStream_t st) {
    hipLaunchKernelGGL(rb_adj_off_kernel, dim3(1), dim3(64), 0, st, d_off, d_count, n_pairs, adj_off);
    if (pl.max_n > 0)
        hipLaunchKernelGGL(rb_graph_kernel, dim3((unsigned)ceil_div64(pl.max_n, RB_GRAPH_BLOCK), (unsigned)n_pairs), dim3(RB_GRAPH_BLOCK),
                           0, st, ms, md, d_off, d_count, 2.0 * c, adj, adj_off, deg);
}

static void rb_launch_clique(const u64 *adj, const int64_t *adj_off, const int32_t *deg, const int64_t *d_off, const int32_t *d_count,
                             int n_pairs, const RbPlan &pl, const RbCliqueWs &ws, int64_t budget, int32_t *clique, int32_t *clique_size,
                             int32_t *certified, int64_t *nodes, hipStream_t st) {
    hipLaunchKernelGGL(rb_prep_kernel, dim3((unsigned)n_pairs), dim3(RB_BLOCK), 0, st, adj, adj_off, deg, d_off, d_count, ws.core_sorted,
                       ws.ord, ws.greedy, ws.state);
    if (pl.max_n > 0) {
        const int64_t words = (int64_t)pl.max_n * ((pl.max_n + 63) / 64);
        hipLaunchKernelGGL(rb_permute_kernel, dim3((unsigned)ceil_div64(words, RB_BLOCK), (unsigned)n_pairs), dim3(RB_BLOCK), 0, st, adj,
                           adj_off, d_off, d_count, ws.ord, ws.adjp);
    }
    hipLaunchKernelGGL(rb_search_kernel, dim3((unsigned)ws.slots, (unsigned)n_pairs), dim3(64), 0, st, ws.adjp, adj_off, ws.core_sorted,
                       d_off, d_count, ws.state, (u64)budget, ws.stack, ws.stack_words, ws.wl, ws.halves, ws.wbest, ws.wkey);
    hipLaunchKernelGGL(rb_clique_final_kernel, dim3((unsigned)n_pairs), dim3(RB_BLOCK), 0, st, d_off, d_count, ws.ord, ws.greedy, ws.state,
                       ws.wbest, ws.wkey, ws.slots, clique, clique_size, certified, nodes);
}

static int rb_common_checks(int n_pairs, double noise_bound, bool with_bound) {
    BATCH_COUNT_CHECK(n_pairs);
    ARG_CHECK(!with_bound || (noise_bound > 0.0 && noise_bound < INFINITY), "noise_bound must be positive and finite");
    return CSLAM_OK;
}

CSLAM_API int cslam_robust_graph_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_count, int n_pairs,
                                     double noise_bound, uint64_t *d_adj, int64_t *d_adj_off, int32_t *d_deg, const int64_t *h_off,
                                     const int32_t *h_count, void *stream) {
    int rc = rb_common_checks(n_pairs, noise_bound, true);
    if (rc) return rc;
    ARG_CHECK(d_ms && d_md && d_off && d_adj && d_adj_off && d_deg, "NULL argument");
    RB_PLAN(pl, d_off, d_count, h_off, h_count, n_pairs, d_ms);
    rb_launch_graph(d_ms, d_md, d_off, d_count, n_pairs, pl, noise_bound, (u64 *)d_adj, d_adj_off, d_deg, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_robust_clique_dev(const uint64_t *d_adj, const int64_t *d_adj_off, const int32_t *d_deg, const int64_t *d_off,
                                      const int32_t *d_count, int n_pairs, int64_t node_budget, int32_t *d_clique,
                                      int32_t *d_clique_size, int32_t *d_certified, int64_t *d_nodes, const int64_t *h_off,
                                      const int32_t *h_count, void *stream) {
    int rc = rb_common_checks(n_pairs, 0.0, false);
    if (rc) return rc;
    ARG_CHECK(node_budget >= 1, "node_budget must be at least 1");
    ARG_CHECK(d_adj && d_adj_off && d_deg && d_off && d_clique && d_clique_size && d_certified, "NULL argument");
    RB_PLAN(pl, d_off, d_count, h_off, h_count, n_pairs, d_adj);
    RbCliqueWs ws;
    auto layout = [&](Carver &cv) { rb_clique_carve(cv, pl, n_pairs, &ws); };
    SCRATCH_CARVE(g_robust_scratch, st, (size_t)1 << 20, layout);
    rb_launch_clique((const u64 *)d_adj, d_adj_off, d_deg, d_off, d_count, n_pairs, pl, ws, node_budget, d_clique, d_clique_size,
                     d_certified, d_nodes, st);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_robust_rotation_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_clique,
                                        const int32_t *d_clique_size, int n_pairs, double noise_bound, double *d_R, double *d_weights,
                                        int32_t *d_iters, const int64_t *h_off, void *stream) {
    int rc = rb_common_checks(n_pairs, noise_bound, true);
    if (rc) return rc;
    ARG_CHECK(d_ms && d_md && d_off && d_clique && d_clique_size && d_R && d_weights && d_iters, "NULL argument");
    if ((rc = rb_host_checks(h_off, nullptr, n_pairs))) return rc;
    PTR_DEVICE(d_ms);
    double nb2 = 4.0 * noise_bound * noise_bound;
    if (nb2 < 1e-16) nb2 = 1e-2;
    hipLaunchKernelGGL(rb_rotation_kernel, dim3((unsigned)n_pairs), dim3(RB_BLOCK), 0, (hipStream_t)stream, d_ms, d_md, d_off, d_clique,
                       d_clique_size, nb2, d_R, d_weights, d_iters);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_robust_translation_dev(const double *d_ms, const double *d_md, const int64_t *d_off, const int32_t *d_clique,
                                           const int32_t *d_clique_size, const double *d_R, int n_pairs, double noise_bound,
                                           double *d_t, int32_t *d_set, const int64_t *h_off, void *stream) {
    int rc = rb_common_checks(n_pairs, noise_bound, true);
    if (rc) return rc;
    ARG_CHECK(d_ms && d_md && d_off && d_clique && d_clique_size && d_R && d_t, "NULL argument");
    RB_PLAN(pl, d_off, (const int32_t *)nullptr, h_off, (const int32_t *)nullptr, n_pairs, d_ms);
    double *xs, *sorted;
    auto layout = [&](Carver &cv) { xs = cv.take<double>(3 * (size_t)pl.total); sorted = cv.take<double>(6 * (size_t)pl.total, 512); };
    SCRATCH_CARVE(g_robust_scratch, st, (size_t)1 << 20, layout);
    hipLaunchKernelGGL(rb_translation_kernel, dim3(3, (unsigned)n_pairs), dim3(RB_BLOCK), 0, st, d_ms, d_md, d_off, d_clique,
                       d_clique_size, d_R, noise_bound, pl.total, xs, sorted, d_t, d_set);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}

CSLAM_API int cslam_robust_fit_dev(const double *d_src, const int64_t *d_src_off, const double *d_dst, const int64_t *d_dst_off,
                                   const int32_t *d_rows, const int64_t *d_row_off, const int32_t *d_count, int n_pairs,
                                   double noise_bound, int64_t node_budget, double *d_T, int64_t *d_info, int32_t *d_clique,
                                   const int64_t *h_row_off, const int32_t *h_count, void *stream) {
    int rc = rb_common_checks(n_pairs, noise_bound, true);
    if (rc) return rc;
    ARG_CHECK(node_budget >= 1, "node_budget must be at least 1");
    ARG_CHECK(d_src && d_src_off && d_dst && d_dst_off && d_rows && d_row_off && d_T && d_info, "NULL argument");
    RB_PLAN(pl, d_row_off, d_count, h_row_off, h_count, n_pairs, d_src);
    const size_t total = (size_t)pl.total;
    RbCliqueWs ws;
    struct Arrays {
        double *ms, *md, *R, *tr, *weights, *xs, *sorted;
        u64 *adj;
        int64_t *adj_off, *nodes;
        int32_t *deg, *clique, *clique_size, *certified, *iters;
    } a;
    auto carve = [&](Carver &cv) {
        a.ms = rb_take<double>(cv, 3 * total); a.md = rb_take<double>(cv, 3 * total);
        a.R = rb_take<double>(cv, 9 * (size_t)n_pairs); a.tr = rb_take<double>(cv, 3 * (size_t)n_pairs);
        a.weights = rb_take<double>(cv, total); a.xs = rb_take<double>(cv, 3 * total); a.sorted = rb_take<double>(cv, 6 * total);
        a.adj = rb_take<u64>(cv, (size_t)pl.adj_words);
        a.adj_off = rb_take<int64_t>(cv, (size_t)n_pairs + 1); a.nodes = rb_take<int64_t>(cv, (size_t)n_pairs);
        a.deg = rb_take<int32_t>(cv, total); a.clique = rb_take<int32_t>(cv, total);
        a.clique_size = rb_take<int32_t>(cv, (size_t)n_pairs); a.certified = rb_take<int32_t>(cv, (size_t)n_pairs);
        a.iters = rb_take<int32_t>(cv, (size_t)n_pairs);
        rb_clique_carve(cv, pl, n_pairs, &ws);
    };
    SCRATCH_CARVE(g_robust_scratch, st, (size_t)1 << 20, carve);
    int32_t *clique = d_clique ? d_clique : a.clique;
    if (pl.max_n > 0)
        hipLaunchKernelGGL(rb_gather_kernel, dim3((unsigned)ceil_div64(pl.max_n, RB_BLOCK), (unsigned)n_pairs), dim3(RB_BLOCK), 0, st, d_src,
                           d_src_off, d_dst, d_dst_off, d_rows, d_row_off, d_count, a.ms, a.md);
    rb_launch_graph(a.ms, a.md, d_row_off, d_count, n_pairs, pl, noise_bound, a.adj, a.adj_off, a.deg, st);
    rb_launch_clique(a.adj, a.adj_off, a.deg, d_row_off, d_count, n_pairs, pl, ws, node_budget, clique, a.clique_size, a.certified,
                     a.nodes, st);
    double nb2 = 4.0 * noise_bound * noise_bound;
    if (nb2 < 1e-16) nb2 = 1e-2;
    hipLaunchKernelGGL(rb_rotation_kernel, dim3((unsigned)n_pairs), dim3(RB_BLOCK), 0, st, a.ms, a.md, d_row_off, clique, a.clique_size,
                       nb2, a.R, a.weights, a.iters);
    hipLaunchKernelGGL(rb_translation_kernel, dim3(3, (unsigned)n_pairs), dim3(RB_BLOCK), 0, st, a.ms, a.md, d_row_off, clique,
                       a.clique_size, a.R, noise_bound, pl.total, a.xs, a.sorted, a.tr, (int32_t *)nullptr);
    hipLaunchKernelGGL(rb_assemble_kernel, dim3((unsigned)ceil_div64(n_pairs, 64)), dim3(64), 0, st, d_row_off, d_count, n_pairs,
                       a.clique_size, a.certified, a.nodes, a.R, a.tr, a.iters, d_T, d_info);
    HIP_TRY(hipGetLastError());
    return CSLAM_OK;
}
