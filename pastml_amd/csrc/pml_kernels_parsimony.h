// Maximum parsimony on packed state sets (pastml/parsimony.py: uppass :92-122, acctran :125-158, downpass :161-210, deltran
// :213-242, the step count :360-380).  Integer work only; every result is independent of the launch geometry.
//
// A state set is W = ceil(k / 64) words per (column, node).  All passes are one primitive: count, per state, in how many of
// a few sets it occurs, and keep the states of a candidate set with the largest count.  The counts are bit-sliced: plane j
// holds bit j of every state's count and a set is added with a ripple carry over the planes (PmlPlanes::add), so the arg-max
// needs no loop over the states -- from the top plane down the candidates become `candidates & plane` wherever that is not
// empty over all W words, and the planes that were kept spell the maximum (most_common).  P planes count up to 2^P - 1: the
// launcher picks P from the forest's largest number of children, there is no cap on the arity.
//
// Lanes: WG = 1, 2, 4 or 8 consecutive lanes (the power of two from W on) own one (node, column), a word each; "not empty
// over all words" is an OR over the group.  Consecutive groups take consecutive units of a level inside a column (blockIdx.y),
// so a wavefront's own sets are contiguous and, children being contiguous ids, its child reads nearly so.
//
// Levels: a launch walks the levels l0 .. l1 - 1 of its pass.  One level may be spread over many workgroups; several levels
// go into one launch of ONE workgroup per column with a barrier between them (the thin ends of a forest: a caterpillar's
// 10^4 levels are a handful of launches).
#pragma once
#include "pml_device.h"

#define PML_PARS_THREADS 256

enum { PML_PARS_UP = 0, PML_PARS_RESTRICT = 1, PML_PARS_DOWN = 2, PML_PARS_STEPS = 3 };

struct PmlParsArgs {
    const int *parent, *first_child, *n_children;
    const int* list;      // the units of the levels: internal nodes by height (UP, STEPS) or by depth (DOWN); null: node ids (RESTRICT)
    const int* offsets;   // the level table of the pass: level l = units offsets[l] .. offsets[l + 1] - 1
    int N, W, WG;
    u64 last_word;        // the states of the last word
    // [column][node][W], the library's numbering
    const u64* init;      // UP, DOWN: the sets the passes start from (annotations; all states where there is none)
    const u64* src;       // UP: unused; RESTRICT: the node's own set; DOWN: the bottom-up sets; STEPS: the sets to count on
    u64* dst;             // UP: bottom-up sets (in place); RESTRICT: result (the parent's is read here); DOWN: final sets; STEPS: Z
    u64* up;              // DOWN: the "up" sets
    i64* m;               // STEPS: [column][node] minimal cost
};

template <int P>
struct PmlPlanes {
    u64 p[P];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < P; ++j) p[j] = 0;
    }
    __device__ __forceinline__ void add(u64 x) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const u64 t = p[j] & x;
            p[j] ^= x;
            x = t;
        }
    }
    // x must have been added before: no count goes below zero
    __device__ __forceinline__ void sub(u64 x) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const u64 t = ~p[j] & x;
            p[j] ^= x;
            x = t;
        }
    }
};

__device__ __forceinline__ int pars_group_or(int v, int WG) {
    for (int o = WG >> 1; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// the states of cand with the largest count; maxv: that count
template <int P>
__device__ __forceinline__ u64 pars_most_common(const PmlPlanes<P>& c, u64 cand, int WG, unsigned& maxv) {
    maxv = 0;
#pragma unroll
    for (int j = P - 1; j >= 0; --j) {
        const u64 t = cand & c.p[j];
        if (pars_group_or(t != 0 ? 1 : 0, WG)) {
            cand = t;
            maxv |= 1u << j;
        }
    }
    return cand;
}

// own & wanted where that is not empty, else own (parsimony.py: `node_states & parent_states or node_states`)
__device__ __forceinline__ u64 pars_restrict(u64 own, u64 wanted, int WG) {
    const u64 both = own & wanted;
    return pars_group_or(both != 0 ? 1 : 0, WG) ? both : own;
}

template <int PASS, int P>
__device__ __forceinline__ void pars_unit(const PmlParsArgs& a, size_t base, int n, int w, bool live, u64 all) {
    const int W = a.W, WG = a.WG;
    unsigned maxv;
    if (PASS == PML_PARS_RESTRICT) {
        const int par = a.parent[n];
        u64 own = live ? a.src[(base + n) * W + w] : 0;
        if (par >= 0) own = pars_restrict(own, live ? a.dst[(base + par) * W + w] : 0, WG);
        if (live) a.dst[(base + n) * W + w] = own;
        return;
    }
    const int fc = a.first_child[n], nc = a.n_children[n];
    PmlPlanes<P> cnt;
    cnt.clear();
    if (PASS == PML_PARS_UP) {
        for (int c = 0; c < nc; ++c) cnt.add(live ? a.dst[(base + fc + c) * W + w] : 0);
        const u64 mc = pars_most_common<P>(cnt, all, WG, maxv);
        const u64 own = live ? a.init[(base + n) * W + w] : 0;
        const u64 res = pars_restrict(own, mc, WG);
        if (live) a.dst[(base + n) * W + w] = res;
    } else if (PASS == PML_PARS_STEPS) {
        i64 msum = 0;
        for (int c = 0; c < nc; ++c) {
            cnt.add(live ? a.dst[(base + fc + c) * W + w] : 0);
            if (w == 0) msum += a.m[base + fc + c];
        }
        const u64 own = live ? a.src[(base + n) * W + w] : 0;
        const u64 z = pars_most_common<P>(cnt, own, WG, maxv);
        if (live) a.dst[(base + n) * W + w] = z;
        if (w == 0) a.m[base + n] = msum + nc - (i64)maxv;
    } else {  // PML_PARS_DOWN
        const int par = a.parent[n];
        cnt.add(par < 0 ? all : (live ? a.up[(base + n) * W + w] : 0));
        for (int c = 0; c < nc; ++c) cnt.add(live ? a.src[(base + fc + c) * W + w] : 0);
        const u64 mc = pars_most_common<P>(cnt, all, WG, maxv);
        const u64 res = pars_restrict(live ? a.init[(base + n) * W + w] : 0, mc, WG);
        if (live) a.dst[(base + n) * W + w] = res;
        for (int c = 0; c < nc; ++c) {
            PmlPlanes<P> t = cnt;
            t.sub(live ? a.src[(base + fc + c) * W + w] : 0);
            const u64 upc = pars_most_common<P>(t, all, WG, maxv);
            if (a.n_children[fc + c] > 0) {
                if (live) a.up[(base + fc + c) * W + w] = upc;
            } else {
                const u64 r = pars_restrict(live ? a.init[(base + fc + c) * W + w] : 0, upc, WG);
                if (live) a.dst[(base + fc + c) * W + w] = r;
            }
        }
    }
}

// grid (x, columns); gridDim.x > 1 only with l1 == l0 + 1
template <int PASS, int P>
__global__ void __launch_bounds__(PML_PARS_THREADS) pars_levels_kernel(PmlParsArgs a, int l0, int l1) {
    const int WG = a.WG;
    const int w = threadIdx.x % WG;
    const bool live = w < a.W;
    const u64 all = !live ? 0 : (w == a.W - 1 ? a.last_word : ~0ull);
    const size_t base = (size_t)blockIdx.y * a.N;
    const int per_block = PML_PARS_THREADS / WG;
    for (int l = l0; l < l1; ++l) {
        const int first = a.offsets[l], end = a.offsets[l + 1];
        for (int q = first + blockIdx.x * per_block + threadIdx.x / WG; q < end; q += gridDim.x * per_block)
            pars_unit<PASS, P>(a, base, a.list ? a.list[q] : q, w, live, all);
        if (l + 1 < l1) {
            __threadfence_block();
            __syncthreads();
        }
    }
}

// annotations in the caller's numbering -> starting sets in the library's (all states where a node has none)
__global__ void pars_init_kernel(const u64* given, u64* init, const int* old_of_new, int N, int W, u64 last_word, int n_cols) {
    const size_t total = (size_t)n_cols * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t col = i / N;
        const int n = (int)(i - col * N);
        const int old = old_of_new ? old_of_new[n] : n;
        const u64* g = given + (col * N + old) * W;
        u64 any = 0;
        for (int w = 0; w < W; ++w) any |= g[w];
        for (int w = 0; w < W; ++w) init[i * W + w] = any ? g[w] : (w == W - 1 ? last_word : ~0ull);
    }
}

// sets in the library's numbering -> the caller's
__global__ void pars_gather_kernel(const u64* sets, u64* out, const int* new_of_old, int N, int W, int n_cols) {
    const size_t total = (size_t)n_cols * N;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t col = i / N;
        const int old = (int)(i - col * N);
        const int n = new_of_old ? new_of_old[old] : old;
        for (int w = 0; w < W; ++w) out[i * W + w] = sets[(col * N + n) * W + w];
    }
}

// nodes by the number of states of their set, per column: hist[column][k + 1].  A workgroup counts in LDS and adds what it
// found with integer atomics (the sums do not depend on the order).  grid (x, columns), (k + 1) ints of dynamic LDS.
__global__ void pars_hist_kernel(const u64* sets, u64* hist, int N, int W, int k) {
    extern __shared__ int pars_lds[];
    for (int s = threadIdx.x; s <= k; s += blockDim.x) pars_lds[s] = 0;
    __syncthreads();
    const u64* col = sets + (size_t)blockIdx.y * N * W;
    for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        int size = 0;
        for (int w = 0; w < W; ++w) size += __popcll(col[(size_t)n * W + w]);
        atomicAdd(&pars_lds[size], 1);
    }
    __syncthreads();
    for (int s = threadIdx.x; s <= k; s += blockDim.x)
        if (pars_lds[s]) atomicAdd(&hist[(size_t)blockIdx.y * (k + 1) + s], (u64)pars_lds[s]);
}

// steps[column] = sum over the roots (node ids first .. first + n_roots - 1) of their minimal cost
__global__ void pars_root_steps_kernel(const i64* m, u64* steps, int N, int first, int n_roots) {
    u64 sum = 0;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < n_roots; r += gridDim.x * blockDim.x)
        sum += (u64)m[(size_t)blockIdx.y * N + first + r];
    if (sum) atomicAdd(&steps[blockIdx.y], sum);
}
