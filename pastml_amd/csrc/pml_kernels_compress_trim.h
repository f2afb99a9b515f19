// Trimming of a horizontally merged forest (pastml/visualisation/tree_compressor.py: compress_tree :118-159, remove_small_tips
// :214-248, remove_mediators :301-340) over its live vertices, entries in Pajek pre-order: parent[i] < i, and the subtree of i
// is the run [i, i + size[i]).  One call; the trees of the forest side by side, each with a threshold of its own.
//
//   sizes      mult[i] = the product of the widths from the root down to i, by pointer jumping with products on copies
//              (2^rounds >= the levels); tsize[i] = (T[i] / w[i]) * mult[i] in float64, the reference's operations in its
//              order.  Products of integers are exact below 2^53 in any order; 2^53 and more raise the error flag.
//   candidates child_max[p] = max tsize of p's children by a 64-bit atomicMax on the bit patterns (non-negative doubles order
//              as their bit patterns do); a non-root vertex with tsize > child_max is a candidate for the threshold.  The
//              k-th largest candidate of every tree is taken on the host from one download of the candidate values.
//   removal    a vertex survives iff it is a root or its run holds a vertex with tsize >= threshold: an inclusive prefix
//              count of those vertices, in three launches -- per-tile totals, their scan by one workgroup, the tiles again
//              with their offsets -- so nothing waits for another workgroup and the result is independent of their order.
//   mediators  n is a candidate iff it survives, is no root, w == 1, T == 0 and exactly one child survives.  Candidates form
//              chains, each the only surviving child of the one above; the group of lanes that finds itself at a chain's
//              bottom walks it upwards, carrying the effective child (the nearest vertex below that is not spliced out):
//              n is spliced out iff in every column |states(n)| >= 2 and states(n) == states(child) | states(parent).
//              WG = 1, 2, 4 or 8 lanes own a vertex, a word each, as in the vertical collapse.  Linear work, one launch.
//   parents    new_parent[i] = the nearest vertex above that is not spliced out; moved[i] = it is not parent[i].
// Integer and exactly rounded work only: every result is independent of the launch geometry.
#pragma once
#include "pml_device.h"

#define PML_TRIM_THREADS 256
#define PML_TRIM_ITEMS 4
#define PML_TRIM_TILE PML_TRIM_SCAN_TILE   // (pml_launch.h) entries of one workgroup of the scan: threads x items

#define PML_TRIM_EXACT 9007199254740992.0   // 2^53

struct TrimForest {
    const int* parent;          // [L] entry above, -1 for a root
    const int* tree;            // [L]
    const int* T;               // [L] tips inside over all configurations
    const int* w;               // [L] width
    const int* size;            // [L] entries of the subtree
    const unsigned char* on;    // [n_trees] the tree is trimmed (sizes: it is over the gate; later: it has a threshold)
    int L;
};

__global__ void trim_mult_init_kernel(TrimForest f, double* mult, int* up) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.L) return;
    mult[i] = (double)f.w[i];
    up[i] = f.parent[i];
}

// One round on copies: after r rounds mult[i] is the product over i and the 2^r - 1 entries above it, up[i] the entry 2^r above.
__global__ void trim_mult_kernel(const double* mult_in, const int* up_in, double* mult_out, int* up_out, int L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L) return;
    const int u = up_in[i];
    mult_out[i] = u >= 0 ? mult_in[i] * mult_in[u] : mult_in[i];
    up_out[i] = u >= 0 ? up_in[u] : -1;
}

// tsize, and the maximum over the children of every vertex (child_max zeroed on entry).
__global__ void trim_tsize_kernel(TrimForest f, const double* mult, double* tsize, unsigned long long* child_max, int* error) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.L) return;
    double ts = 0.;
    if (f.on[f.tree[i]]) {
        const double m = mult[i];
        ts = ((double)f.T[i] / (double)f.w[i]) * m;
        if (!(m < PML_TRIM_EXACT) || !(ts < PML_TRIM_EXACT)) atomicExch(error, 1);
        const int p = f.parent[i];
        if (p >= 0) atomicMax(&child_max[p], (unsigned long long)__double_as_longlong(ts));
    }
    tsize[i] = ts;
}

// candidate[i] = tsize[i] where i is a candidate for its tree's threshold, else -1.
__global__ void trim_candidates_kernel(TrimForest f, const double* tsize, const unsigned long long* child_max, double* candidate) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.L) return;
    const double ts = tsize[i];
    const bool is = f.on[f.tree[i]] && f.parent[i] >= 0 && ts > __longlong_as_double((long long)child_max[i]);
    candidate[i] = is ? ts : -1.;
}

__device__ __forceinline__ int trim_big(const TrimForest& f, const double* tsize, const double* threshold, int i) {
    const int t = f.tree[i];
    return f.on[t] && tsize[i] >= threshold[t];
}

// Sum of v over the workgroup's threads, in every thread; and the exclusive prefix of the thread's own v in *before.
__device__ __forceinline__ int trim_block_scan(int v, int* before) {
    __shared__ int wave_total[PML_TRIM_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    int offset = 0, total = 0;
    for (int j = 0; j < PML_TRIM_THREADS / 64; ++j) {
        const int x = wave_total[j];
        if (j < wave) offset += x;
        total += x;
    }
    __syncthreads();   // (the array is free for the next call)
    *before = offset + incl - v;
    return total;
}

// Phase 1: the number of big vertices in every tile.
__global__ void __launch_bounds__(PML_TRIM_THREADS)
trim_scan_totals_kernel(TrimForest f, const double* tsize, const double* threshold, int* tile_total) {
    const long long base = (long long)blockIdx.x * PML_TRIM_TILE + (long long)threadIdx.x * PML_TRIM_ITEMS;
    int v = 0;
    for (int j = 0; j < PML_TRIM_ITEMS; ++j)
        if (base + j < f.L) v += trim_big(f, tsize, threshold, (int)(base + j));
    int before;
    const int total = trim_block_scan(v, &before);
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// Phase 2: tile_total becomes its exclusive prefix sum; one workgroup walks the tiles, PML_TRIM_THREADS at a time, with a carry.
__global__ void __launch_bounds__(PML_TRIM_THREADS)
trim_scan_tiles_kernel(int* tile_total, int n_tiles) {
    int carry = 0;
    for (int b0 = 0; b0 < n_tiles; b0 += PML_TRIM_THREADS) {   // (uniform: every thread runs every round)
        const int b = b0 + (int)threadIdx.x;
        const int v = b < n_tiles ? tile_total[b] : 0;
        int before;
        const int total = trim_block_scan(v, &before);
        if (b < n_tiles) tile_total[b] = carry + before;
        carry += total;
    }
}

// Phase 3: incl[i] = the number of big vertices among the entries 0 .. i.
__global__ void __launch_bounds__(PML_TRIM_THREADS)
trim_scan_write_kernel(TrimForest f, const double* tsize, const double* threshold, const int* tile_before, int* incl) {
    const long long base = (long long)blockIdx.x * PML_TRIM_TILE + (long long)threadIdx.x * PML_TRIM_ITEMS;
    int big[PML_TRIM_ITEMS];
    int v = 0;
    for (int j = 0; j < PML_TRIM_ITEMS; ++j) {
        big[j] = base + j < f.L ? trim_big(f, tsize, threshold, (int)(base + j)) : 0;
        v += big[j];
    }
    int before;
    trim_block_scan(v, &before);
    int run = tile_before[blockIdx.x] + before;
    for (int j = 0; j < PML_TRIM_ITEMS; ++j) {
        run += big[j];
        if (base + j < f.L) incl[base + j] = run;
    }
}

// keep[i], and for the survivors the number of surviving children of their parents and one of them (n_kept zeroed on entry).
// The run of i ends at i + size[i] - 1 < L (checked on the host).
__global__ void trim_keep_kernel(TrimForest f, const double* tsize, const double* threshold, const int* incl, unsigned char* keep,
                                 int* n_kept, int* only) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.L) return;
    const int p = f.parent[i];
    bool k = true;
    if (f.on[f.tree[i]] && p >= 0) {
        const int inside = incl[i + f.size[i] - 1] - incl[i] + trim_big(f, tsize, threshold, i);
        k = inside > 0;
    }
    keep[i] = k;
    if (k && p >= 0) {
        atomicAdd(&n_kept[p], 1);
        only[p] = i;   // (read only where n_kept[p] == 1: then this is the one store)
    }
}

__device__ __forceinline__ bool trim_structural(const TrimForest& f, const unsigned char* keep, const int* n_kept, int i) {
    return f.on[f.tree[i]] && keep[i] && f.parent[i] >= 0 && f.w[i] == 1 && f.T[i] == 0 && n_kept[i] == 1;
}

// sets: [n_cols][L][W].  A group of WG lanes per entry; the group of a chain's bottom walks the chain.  The lanes of a group
// take every branch together (what they branch on is the same in all of them), so the shuffles stay inside the group.
__global__ void __launch_bounds__(PML_TRIM_THREADS)
trim_chain_kernel(TrimForest f, const u64* sets, const unsigned char* keep, const int* n_kept, const int* only, unsigned char* spliced,
                  int W, int WG, int n_cols) {
    const int lane = threadIdx.x % WG;
    const long long i = (long long)blockIdx.x * (PML_TRIM_THREADS / WG) + threadIdx.x / WG;
    if (i >= f.L) return;
    if (!trim_structural(f, keep, n_kept, (int)i)) return;
    int below = only[i];
    if (trim_structural(f, keep, n_kept, below)) return;   // not the bottom of its chain
    const size_t col_words = (size_t)f.L * W;
    int n = (int)i;
    for (;;) {
        const int p = f.parent[n];   // (>= 0: n is a candidate)
        int fits = 1;
        for (int c = 0; c < n_cols && fits; ++c) {
            int same = 1, bits = 0;
            if (lane < W) {
                const u64* col = sets + c * col_words + lane;
                const u64 own = col[(size_t)n * W];
                same = own == (col[(size_t)below * W] | col[(size_t)p * W]);
                bits = __popcll(own);
            }
            for (int o = WG >> 1; o > 0; o >>= 1) {
                same &= __shfl_xor(same, o);
                bits += __shfl_xor(bits, o);
            }
            fits = same && bits >= 2;
        }
        if (fits) {
            if (lane == 0) spliced[n] = 1;
        } else {
            below = n;
        }
        if (!trim_structural(f, keep, n_kept, p)) break;
        n = p;   // (n is p's only surviving child: p's chain is this one)
    }
}

// new_parent and moved (spliced is complete).  A vertex that is gone or spliced out gets -1 / 0.
__global__ void trim_parents_kernel(TrimForest f, const unsigned char* keep, const unsigned char* spliced, int* new_parent,
                                    unsigned char* moved) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= f.L) return;
    int p = -1;
    unsigned char m = 0;
    if (keep[i] && !spliced[i]) {
        p = f.parent[i];
        while (p >= 0 && spliced[p]) p = f.parent[p];
        m = p != f.parent[i];
    }
    new_parent[i] = p;
    moved[i] = m;
}
