// Timeline of the compressed map (pastml/tree.py: annotate_dates :51-65; pastml/visualisation/cytoscape_manager.py: the get_date
// of visualize :751-762, the milestone loop of _forest2json_compressed :219-268) over a forest given as arrays.  Node ids are
// breadth-first: level d is the run [level[d], level[d + 1]) and a parent's id is smaller than its children's.
//
//   dates      date[n] = given[n], else the root's date, else date[parent] + dist[n]: ONE addition per node in the order of the
//              reference, so the bits are its bits (milestones are dates and the counts compare date <= milestone).  Level by
//              level from the roots; consecutive levels of at most PML_TL_FUSE nodes share a launch of one workgroup with a
//              barrier between them.
//   get_date   NODES: date; LTT: date[up] + 1e-6 below a root; SAMPLED: the minimum date over the alive tips below, a 64-bit
//              atomicMin on an order-preserving encoding of the doubles, level by level from the deepest (the same fusing) --
//              a minimum is exact in any order -- and the maximum over all tips where there is none.
//   bins       bin[n] = the first milestone >= get_date[n] (M: none), by binary search over the milestones in LDS;
//              cbin[x] = min of that over the alive nodes whose up is x, an integer atomicMin.  (LTT: see tl_bins_kernel.)
//   counts     per configuration difference arrays [C, M + 1] filled with integer atomics: an alive tip is +1 at bin; an alive
//              internal node is a tip on [bin, cbin) and an internal node from max(bin, cbin) on.  A running sum along the
//              milestones turns them into the counts.
//   below      the tips in left-to-right leaf order: those of a subtree are a run [lo, hi).  Per tile of PML_TL_TILE tips a
//              histogram of their bins, an exclusive running sum over the tiles, and per configuration the two partial tiles
//              at the ends of its run; a running sum along the milestones.
//   vertices   a workgroup per vertex: lane = milestone, the wavefronts stride over the members; count, min and max.
// Integer work, one addition and minima only: every result is independent of the launch geometry.
#pragma once
#include "pml_device.h"

#define PML_TL_THREADS 256
#define PML_TL_FUSE PML_TL_FUSE_WIDTH   // (pml_launch.h) levels of at most this many nodes, two per thread, may share a launch
#define PML_TL_TILE 1024       // tips of one tile of the prefix counts
#define PML_TL_MAX_M 64
#define PML_TL_NEVER 0x7f7f7f7f   // cbin of a node without alive children (what a memset of 0x7f leaves)

#define PML_TL_SAMPLED 0
#define PML_TL_NODES 1
#define PML_TL_LTT 2

typedef unsigned long long tl_u64;

// doubles in the order of their values as unsigned integers
__device__ __forceinline__ tl_u64 tl_encode(double x) {
    const tl_u64 b = (tl_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double tl_decode(tl_u64 e) {
    const tl_u64 b = (e >> 63) ? (e & 0x7fffffffffffffffull) : ~e;
    return __longlong_as_double((long long)b);
}

__device__ __forceinline__ void tl_date_of(int n, const int* parent, const double* dist, const double* given, const double* root_dates,
                                           double* date) {
    const double g = given[n];
    const int p = parent[n];
    date[n] = g == g ? g : (p < 0 ? root_dates[n] : date[p] + dist[n]);
}

// one level [a, b): its parents are complete
__global__ void tl_dates_level_kernel(int a, int b, const int* parent, const double* dist, const double* given,
                                      const double* root_dates, double* date) {
    const int n = a + blockIdx.x * blockDim.x + threadIdx.x;
    if (n < b) tl_date_of(n, parent, dist, given, root_dates, date);
}

// levels [d0, d1), each of at most PML_TL_FUSE nodes: one workgroup, a barrier between the levels
__global__ void tl_dates_fused_kernel(int d0, int d1, const int* level, const int* parent, const double* dist, const double* given,
                                      const double* root_dates, double* date) {
    for (int d = d0; d < d1; ++d) {
        const int b = level[d + 1];
        for (int n = level[d] + threadIdx.x; n < b; n += blockDim.x) tl_date_of(n, parent, dist, given, root_dates, date);
        __syncthreads();
    }
}

// smin[n] = the encoded date of an alive tip, else the largest code; *max_code = the largest code of a tip (zeroed on entry)
__global__ void tl_sampled_init_kernel(int N, const double* date, const unsigned char* alive, const unsigned char* is_tip, tl_u64* smin,
                                       tl_u64* max_code) {
    __shared__ tl_u64 s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) {
        const tl_u64 e = tl_encode(date[n]);
        smin[n] = (alive[n] && is_tip[n]) ? e : ~0ull;
        if (is_tip[n]) atomicMax(&s_max, e);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(max_code, s_max);
}

// (the minima arrive by atomics, which are carried out in L2: an atomic load reads them there too, not from a line that this
// compute unit cached while an earlier level of the same launch read its neighbours)
__device__ __forceinline__ void tl_min_up(int n, const int* parent, tl_u64* smin) {
    const int p = parent[n];
    const tl_u64 e = __hip_atomic_load(&smin[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p >= 0 && e != ~0ull) atomicMin(&smin[p], e);
}

__global__ void tl_sampled_level_kernel(int a, int b, const int* parent, tl_u64* smin) {
    const int n = a + blockIdx.x * blockDim.x + threadIdx.x;
    if (n < b) tl_min_up(n, parent, smin);
}

// levels d1 - 1 down to d0, each of at most PML_TL_FUSE nodes
__global__ void tl_sampled_fused_kernel(int d0, int d1, const int* level, const int* parent, tl_u64* smin) {
    for (int d = d1 - 1; d >= d0; --d) {
        const int b = level[d + 1];
        for (int n = level[d] + threadIdx.x; n < b; n += blockDim.x) tl_min_up(n, parent, smin);
        __syncthreads();
    }
}

__global__ void tl_get_date_kernel(int N, int type, const double* date, const int* up, const tl_u64* smin, const tl_u64* max_code,
                                   double* get_date) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double g;
    if (type == PML_TL_NODES) {
        g = date[n];
    } else if (type == PML_TL_LTT) {
        const int u = up[n];
        g = u < 0 ? date[n] : date[u] + 1e-6;
    } else {
        const tl_u64 e = smin[n];
        g = tl_decode(e == ~0ull ? *max_code : e);
    }
    get_date[n] = g;
}

// the first i with x <= m[i], M if there is none (m ascending, in LDS)
__device__ __forceinline__ int tl_bin_of(double x, const double* m, int M) {
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x <= m[mid]) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// bin of every node, and the minimum over the alive children in the up tree (cbin: PML_TL_NEVER on entry).  A child is in the
// tree from the bin of its get_date on, and that is what cbin takes.  The lists of a vertex show a node from bin[n] on, which
// under LTT is the earlier of that and the bin of its own date: the reference asks a node that it has cut out of the tree --
// a root by then -- for its date, not for its parent's (a difference only where a branch is shorter than 1e-6).
__global__ void tl_bins_kernel(int N, int M, int type, const double* milestones, const double* date, const double* get_date,
                               const unsigned char* alive, const int* up, int* bin, int* cbin) {
    __shared__ double m[PML_TL_MAX_M];
    if (threadIdx.x < M) m[threadIdx.x] = milestones[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int b = tl_bin_of(get_date[n], m, M);
    const int u = up[n];
    bin[n] = (type == PML_TL_LTT && u >= 0) ? min(b, tl_bin_of(date[n], m, M)) : b;
    if (alive[n] && u >= 0) atomicMin(&cbin[u], b);
}

// the bins of the tips' own dates, in leaf order
__global__ void tl_tip_bins_kernel(int T, int M, const double* milestones, const double* date, const int* tip_order, unsigned char* tbin) {
    __shared__ double m[PML_TL_MAX_M];
    if (threadIdx.x < M) m[threadIdx.x] = milestones[threadIdx.x];
    __syncthreads();
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < T) tbin[r] = (unsigned char)tl_bin_of(date[tip_order[r]], m, M);
}

// difference arrays of the two roles, [C, M + 1] each, zeroed on entry
__global__ void tl_roles_kernel(int N, int M, const unsigned char* alive, const int* config, const unsigned char* is_tip,
                                const unsigned char* is_polytomy, const int* bin, const int* cbin, int* d_tips, int* d_internal) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int c = config[n];
    if (!alive[n] || c < 0 || is_polytomy[n]) return;
    const size_t row = (size_t)c * (M + 1);
    const int b = bin[n];
    if (is_tip[n]) {
        atomicAdd(&d_tips[row + b], 1);
        return;
    }
    const int cb = min(cbin[n], M);
    if (cb > b) {
        atomicAdd(&d_tips[row + b], 1);
        atomicAdd(&d_tips[row + cb], -1);
    }
    atomicAdd(&d_internal[row + max(b, cb)], 1);
}

// running sums along the milestones, in place
__global__ void tl_roles_sum_kernel(int C, int M, int* d_tips, int* d_internal) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const size_t row = (size_t)c * (M + 1);
    int a = 0, b = 0;
    for (int i = 0; i <= M; ++i) {
        a += d_tips[row + i];
        b += d_internal[row + i];
        d_tips[row + i] = a;
        d_internal[row + i] = b;
    }
}

// hist[tile + 1][j] = tips of the tile in bin j (row 0 is zeroed by the caller; bins >= M are not counted)
__global__ void tl_tile_hist_kernel(int T, int M, const unsigned char* tbin, int* hist) {
    __shared__ int h[PML_TL_MAX_M];
    if (threadIdx.x < PML_TL_MAX_M) h[threadIdx.x] = 0;
    __syncthreads();
    const int begin = blockIdx.x * PML_TL_TILE;
    const int end = min(T, begin + PML_TL_TILE);
    for (int r = begin + threadIdx.x; r < end; r += blockDim.x) {
        const int j = tbin[r];
        if (j < M) atomicAdd(&h[j], 1);
    }
    __syncthreads();
    if (threadIdx.x < PML_TL_MAX_M) hist[(size_t)(blockIdx.x + 1) * PML_TL_MAX_M + threadIdx.x] = h[threadIdx.x];
}

// rows 0 .. n_tiles: row t becomes the tips of the tiles before t, per bin (one workgroup of PML_TL_MAX_M threads)
__global__ void tl_tile_scan_kernel(int n_tiles, int* hist) {
    const int j = threadIdx.x;
    int sum = 0;
    for (int t = 0; t <= n_tiles; ++t) {
        sum += hist[(size_t)t * PML_TL_MAX_M + j];
        hist[(size_t)t * PML_TL_MAX_M + j] = sum;
    }
}

// below[c][i] = tips of the run [lo[c], hi[c]) with a bin <= i; a workgroup per configuration
__global__ void tl_below_kernel(int M, const int* lo, const int* hi, const unsigned char* tbin, const int* hist, int* below) {
    __shared__ int h[PML_TL_MAX_M];
    const int c = blockIdx.x;
    if (threadIdx.x < PML_TL_MAX_M) h[threadIdx.x] = 0;
    __syncthreads();
    const int a = lo[c], b = hi[c];
    const int ta = a / PML_TL_TILE, tb = b / PML_TL_TILE;
    if (ta == tb) {
        for (int r = a + threadIdx.x; r < b; r += blockDim.x) {
            const int j = tbin[r];
            if (j < M) atomicAdd(&h[j], 1);
        }
    } else {
        for (int r = tb * PML_TL_TILE + threadIdx.x; r < b; r += blockDim.x) {
            const int j = tbin[r];
            if (j < M) atomicAdd(&h[j], 1);
        }
        for (int r = ta * PML_TL_TILE + threadIdx.x; r < a; r += blockDim.x) {
            const int j = tbin[r];
            if (j < M) atomicAdd(&h[j], -1);
        }
    }
    __syncthreads();
    if (threadIdx.x < PML_TL_MAX_M)
        h[threadIdx.x] += hist[(size_t)tb * PML_TL_MAX_M + threadIdx.x] - hist[(size_t)ta * PML_TL_MAX_M + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < M) {
        int sum = 0;
        for (int j = 0; j <= (int)threadIdx.x; ++j) sum += h[j];
        below[(size_t)c * M + threadIdx.x] = sum;
    }
}

struct TimelineOut {
    int* n_roots;        // [L, M]
    int* tips_min;
    int* tips_max;
    int* internal_min;
    int* internal_max;
    int* below_min;
    int* below_max;
    int* first;          // [L]
};

// A workgroup of 4 wavefronts per vertex: lane = milestone, the wavefronts stride over the vertex's configurations.
__global__ void tl_vertices_kernel(int M, const int* member_offsets, const int* top, const int* bin, const int* tips, const int* internal,
                                   const int* below, TimelineOut out) {
    __shared__ int s[4][7][PML_TL_MAX_M];
    __shared__ int s_first;
    const int v = blockIdx.x;
    const int i = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_first = M;
    int n = 0, lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {0, 0, 0};
    if (i < M) {
        const int end = member_offsets[v + 1];
        for (int c = member_offsets[v] + w; c < end; c += 4) {
            if (bin[top[c]] > i) continue;
            ++n;
            const int x[3] = {tips[(size_t)c * (M + 1) + i], internal[(size_t)c * (M + 1) + i], below[(size_t)c * M + i]};
            for (int q = 0; q < 3; ++q) {
                lo[q] = min(lo[q], x[q]);
                hi[q] = max(hi[q], x[q]);
            }
        }
    }
    s[w][0][i] = n;
    for (int q = 0; q < 3; ++q) {
        s[w][1 + 2 * q][i] = lo[q];
        s[w][2 + 2 * q][i] = hi[q];
    }
    __syncthreads();
    if (w == 0 && i < M) {
        for (int u = 1; u < 4; ++u) {
            n += s[u][0][i];
            for (int q = 0; q < 3; ++q) {
                lo[q] = min(lo[q], s[u][1 + 2 * q][i]);
                hi[q] = max(hi[q], s[u][2 + 2 * q][i]);
            }
        }
        const size_t at = (size_t)v * M + i;
        out.n_roots[at] = n;
        out.tips_min[at] = n ? lo[0] : 0;
        out.tips_max[at] = hi[0];
        out.internal_min[at] = n ? lo[1] : 0;
        out.internal_max[at] = hi[1];
        out.below_min[at] = n ? lo[2] : 0;
        out.below_max[at] = hi[2];
        if (n) atomicMin(&s_first, i);
    }
    __syncthreads();
    if (threadIdx.x == 0) out.first[v] = s_first;
}
