// Vertical collapse of a reconstructed forest (pastml/visualisation/tree_compressor.py: collapse_vertically :251-298, the
// TIPS_INSIDE / INTERNAL_NODES_INSIDE lists of compress_tree :87-96): a node whose state sets equal its parent's in every
// column belongs to its parent's vertex.  Integer work only; every result is independent of the launch geometry.
//
// Numbering: these kernels work in the CALLER's numbering (level order: the children of a node are consecutive ids, and so
// are the siblings' parents) -- the sets arrive in it, the results leave in it, and the node ids among the results (top,
// parent_vertex) need no mapping back.  compress_tree_kernel makes the two per-node tables they need from the library's.
//
// merged pass: [column][node][W] words; WG = 1, 2, 4 or 8 consecutive lanes (the power of two from W on) own one node, a word
// each, and walk the columns of the chunk.  Consecutive groups take consecutive nodes, so a wavefront's own words of one
// column are one contiguous run; the parent's words are a gather (neighbouring nodes share or neighbour their parents).
// Bytes: 2 * 8 * n_cols * W per node that has a parent (its own words and its parent's), + 4 for the parent id, + 1 flag.
//
// top: top[n] = n for a node that starts a vertex, else its parent; then rounds of top[n] = top[top[n]] (pointer jumping)
// until 2^rounds covers the deepest node -- a caterpillar of 10^6 tips is 20 launches, not 10^6, and no flag is read back.
#pragma once
#include "pml_device.h"

#define PML_COMPRESS_THREADS 256

enum { PML_COMPRESS_TIP = 0, PML_COMPRESS_INTERNAL = 1, PML_COMPRESS_UNCOUNTED = 2 };   // kinds of compress_tree_kernel

// The tree in the caller's numbering: parent[n] (-1: a root) and kind[n] (a tip, an internal node, an internal node that the
// counts leave out: IS_POLYTOMY).  new_of_old / old_of_new: null when the library kept the caller's numbering.
__global__ void compress_tree_kernel(const int* lib_parent, const int* lib_n_children, const int* new_of_old, const int* old_of_new,
                                     const unsigned char* is_polytomy, int* parent, unsigned char* kind, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int lib = new_of_old ? new_of_old[n] : n;
    const int p = lib_parent[lib];
    parent[n] = p < 0 ? -1 : (old_of_new ? old_of_new[p] : p);
    kind[n] = lib_n_children[lib] == 0 ? PML_COMPRESS_TIP
                                       : (is_polytomy && is_polytomy[n] ? PML_COMPRESS_UNCOUNTED : PML_COMPRESS_INTERNAL);
}

// differs[n] |= some word of some column of the chunk is not the parent's.  sets: [n_cols][N][W] of the chunk.  A launch per
// chunk of columns on one stream: the flags of a node are written by one group per launch, and the launches are ordered.
__global__ void __launch_bounds__(PML_COMPRESS_THREADS)
compress_differs_kernel(const u64* sets, const int* parent, unsigned char* differs, int N, int W, int WG, int n_cols) {
    const int w = threadIdx.x % WG;
    const int per_block = PML_COMPRESS_THREADS / WG;
    const size_t col_words = (size_t)N * W;
    for (size_t n = (size_t)blockIdx.x * per_block + threadIdx.x / WG; n < (size_t)N; n += (size_t)gridDim.x * per_block) {
        const int p = parent[n];
        int d = 0;
        if (p >= 0 && w < W) {
            const u64* own = sets + n * W + w;
            const u64* par = sets + (size_t)p * W + w;
            u64 x = 0;
            int c = 0;
            for (; c + 4 <= n_cols; c += 4) {   // (independent loads in flight: the pass is bound by memory latency and bandwidth)
                const u64 a0 = own[c * col_words], a1 = own[(c + 1) * col_words], a2 = own[(c + 2) * col_words],
                          a3 = own[(c + 3) * col_words];
                const u64 b0 = par[c * col_words], b1 = par[(c + 1) * col_words], b2 = par[(c + 2) * col_words],
                          b3 = par[(c + 3) * col_words];
                x |= (a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2) | (a3 ^ b3);
            }
            for (; c < n_cols; ++c) x |= own[c * col_words] ^ par[c * col_words];
            d = x != 0;
        }
        // (the lanes of a group are in or out of the loop together: n depends on threadIdx.x / WG only)
        for (int o = WG >> 1; o > 0; o >>= 1) d |= __shfl_xor(d, o);
        if (d && w == 0) differs[n] = 1;
    }
}

__global__ void compress_top_init_kernel(const int* parent, const unsigned char* differs, int* top, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int p = parent[n];
    top[n] = (p >= 0 && !differs[n]) ? p : n;
}

// One round of pointer jumping, in place.  top[n] is always n or an ancestor of n inside n's vertex, and a round only moves
// it further up inside that vertex; a lane that reads top[t] while another lane is rewriting it sees the old or the new value
// (aligned 32-bit loads and stores do not tear), either of which is such an ancestor at least as far up as the value a
// round on a copy would have read.  So after r rounds top[n] is the vertex's first node or at least 2^r steps up, whatever
// the order of the lanes, and the fixed point -- the first node of the vertex -- is the same.
__global__ void compress_jump_kernel(int* top, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int t = top[n];
    const int tt = top[t];
    if (tt != t) top[n] = tt;
}

// tips_inside[top[n]] / internal_inside[top[n]] += 1 by the kind of n, and parent_vertex[n] = top[parent[n]] where n starts
// a vertex (-1 for a root and for every other node).  COMBINE: a run of neighbouring lanes of a wavefront with the same top
// -- level order keeps the nodes of a vertex together, and one vertex over a whole clade is the common case -- adds its
// two sums with one atomic each, issued by the run's first lane; without it every lane issues its own.  Integer sums: the
// result does not depend on the order or on COMBINE.  The counts must be zero on entry.
template <bool COMBINE>
__global__ void __launch_bounds__(PML_COMPRESS_THREADS)
compress_counts_kernel(const int* top, const int* parent, const unsigned char* kind, int* tips_inside, int* internal_inside,
                       int* parent_vertex, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;   // (no early return: the ballots below want every lane of the wavefront)
    const bool in = n < N;
    const int t = in ? top[n] : -1;
    const int k = in ? kind[n] : PML_COMPRESS_UNCOUNTED;
    if (in) {
        const int p = parent[n];
        parent_vertex[n] = (t == n && p >= 0) ? top[p] : -1;
    }
    if (!COMBINE) {
        if (k == PML_COMPRESS_TIP) atomicAdd(&tips_inside[t], 1);
        else if (k == PML_COMPRESS_INTERNAL) atomicAdd(&internal_inside[t], 1);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(t, 1);
    const u64 heads = __ballot(lane == 0 || before != t);   // the lanes that start a run (blockDim.x is a multiple of 64)
    const u64 tips = __ballot(k == PML_COMPRESS_TIP);
    const u64 internals = __ballot(k == PML_COMPRESS_INTERNAL);
    if (in && ((heads >> lane) & 1)) {
        const u64 above = lane == 63 ? 0 : (heads >> (lane + 1)) << (lane + 1);          // the heads after this one
        const u64 upto = above ? ((above & (~above + 1)) - 1) : ~0ull;                   // lanes below the next head
        const u64 run = upto & (~0ull << lane);
        const int nt = __popcll(tips & run), ni = __popcll(internals & run);
        if (nt) atomicAdd(&tips_inside[t], nt);
        if (ni) atomicAdd(&internal_inside[t], ni);
    }
}
