// Forward simulation of a character along the forest (pastml/utilities/state_simulator.py:6-31) on the device.
//
// Every root draws from pi; every other node draws from row a of its branch's P(t), a = its parent's state in the same
// repetition (negative entries clamped to 0).  Repetitions are independent, and a subtree depends only on its root's state:
// the work is (node list, repetition tile) items.  A thread owns 4 consecutive repetitions of a tile and walks the nodes of
// its list in order (parents before children: a list is one node of a depth level, or a subtree in preorder), so
// the parent's states it reads are ones it wrote itself or ones an earlier launch wrote -- no barrier between nodes.
//
// States are rows per node in the caller's numbering ([node][rep], row stride rs, a multiple of 4): a thread's parent
// read and child write are one 4-byte word (uint8, k <= 256) or 8 bytes (uint16), contiguous across the wavefront.
//
// Draws: one Philox-4x32-10 call keyed by seed, counter (global repetition / 4, caller's node id) gives the 4 uniforms of a
// thread's 4 repetitions, u = x * 2^-32 (32 bits).  Each state's probability is realised as a count of 2^-32 grid points,
// so every cell of a row is off by at most 2^-32 (absolute), which is below anything a test can see at k <= 512.  The result
// is a pure function of (seed, node, global repetition): launch geometry, chunking (rep_offset) and the library's internal
// numbering never show.
//
//   F81 / JC / EFT: P is never formed.  With e = exp(-mu t') of the branch the child keeps the parent's state when u < e,
//                   else draws from pi with (u - e) / (1 - e) -- bisection in the cumulative pi table (LDS).  P(0) = I: a
//                   zero branch copies exactly (e = 1).
//   HKY / JTT / CUSTOM_RATES: the per-branch P(t) of the P(t) batch, stored transposed (Pt[a * ks + b] = P[b][a]).  The
//                   workgroup builds the cumulative rows cdf[a][b] = sum_{b' <= b} max(P[a][b'], 0) of a branch once, in LDS
//                   (k <= PML_SIM_LDS_K) or in a per-workgroup slice of a scratch buffer, then every lane scales u by its
//                   row's sum and bisects.
#pragma once
#include "pml_device.h"
#include "pml_philox.h"

#define PML_SIM_THREADS 256
#define PML_SIM_LDS_K 128          // matrix models: cumulative rows in LDS up to (k^2 + k) * 8 B = 129 KiB
#define PML_SIM_F81 0
#define PML_SIM_MATRIX_LDS 1
#define PML_SIM_MATRIX_SCRATCH 2

struct PmlSimArgs {
    const int* parent;        // internal ids
    const int* api_id;        // caller's id of an internal node (null: the same)
    const int4* lists;        // node lists, entries (internal id, caller's id, caller's id of the parent or -1, slot of the
                              // branch's matrix in the P(t) window: 0 where there is none)
                              // (null: list i is the single node first_node + i, and its slot is i)
    const int* list_off;      // [n_lists + 1]
    int first_node, n_lists;
    int n_tiles;              // repetition tiles per list (blockDim.x tuples each)
    int n_tuples;             // rs / 4
    size_t rs;                // row stride (elements)
    void* states;             // [N][rs], caller's numbering
    unsigned rep_offset;
    u64 seed;
    int k, ks;
    const double* pi;         // [ks] of the column
    const double* E;          // [N] of the column (F81)
    const double* P;          // [N][k][ks] of the column (matrix models); WIN: the column's window [B][k][ks], whose slots hold
                              // the matrices of this launch's nodes (pml_pij_window.h: built right before it)
    double* scratch;          // [gridDim.x][k][k] (PML_SIM_MATRIX_SCRATCH)
};

// the 4 uniforms (as 32-bit integers) of global repetitions g0 .. g0 + 3 of node `key`
__device__ __forceinline__ void sim_bits(u64 seed, unsigned key, unsigned g0, unsigned (&x)[4]) {
    unsigned a[4] = {g0 >> 2, key, 0u, 0x73696d75u};
    philox4x32_10(a, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned sh = g0 & 3u;   // (launch-uniform: rep_offset % 4)
    if (sh == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = a[i];
        return;
    }
    unsigned b[4] = {(g0 >> 2) + 1u, key, 0u, 0x73696d75u};
    philox4x32_10(b, (unsigned)seed, (unsigned)(seed >> 32));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const unsigned j = sh + (unsigned)i;   // word j of block g0 / 4, j - 4 of the next
        unsigned v = b[0];
        v = j == 1u ? a[1] : v;
        v = j == 2u ? a[2] : v;
        v = j == 3u ? a[3] : v;
        v = j == 5u ? b[1] : v;
        v = j == 6u ? b[2] : v;
        x[i] = v;
    }
}

__device__ __forceinline__ double sim_u(unsigned x) { return (double)x * 0x1p-32; }

// first b in [0, k) with cdf[b] > w (the last state if rounding put w at the total)
__device__ __forceinline__ int sim_bisect(const double* cdf, int k, double w) {
    int lo = 0, hi = k - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > w) hi = mid; else lo = mid + 1;
    }
    return lo;
}

template <typename T> struct SimWord;
template <> struct SimWord<unsigned char> {
    typedef unsigned W;
    static __device__ __forceinline__ void unpack(W w, int (&s)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = (int)((w >> (8 * i)) & 0xffu);
    }
    static __device__ __forceinline__ W pack(const int (&s)[4]) {
        return (unsigned)s[0] | ((unsigned)s[1] << 8) | ((unsigned)s[2] << 16) | ((unsigned)s[3] << 24);
    }
};
template <> struct SimWord<unsigned short> {
    typedef uint2 W;
    static __device__ __forceinline__ void unpack(W w, int (&s)[4]) {
        s[0] = (int)(w.x & 0xffffu);
        s[1] = (int)(w.x >> 16);
        s[2] = (int)(w.y & 0xffffu);
        s[3] = (int)(w.y >> 16);
    }
    static __device__ __forceinline__ W pack(const int (&s)[4]) {
        uint2 w;
        w.x = (unsigned)s[0] | ((unsigned)s[1] << 16);
        w.y = (unsigned)s[2] | ((unsigned)s[3] << 16);
        return w;
    }
};

// inclusive scan over the 64 lanes of a wavefront
__device__ __forceinline__ double sim_wave_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double up = __shfl_up(v, o, 64);
        if (lane >= o) v += up;
    }
    return v;
}

// Items (list, tile) in a grid-stride loop over blockIdx.x; all threads of a workgroup take the same item (the matrix
// models share the branch's cumulative rows).  Dynamic LDS: cumulative pi [k], then (MATRIX_LDS) the rows [k][k].
// 8 waves per SIMD: at the compiler's own choice (101 SGPRs, 7 waves) a subtree walk of 2048 workgroups ran in more than one
// round (profiles/simulate_scale.txt); the SGPRs beyond spill into VGPR lanes, not scratch.
// WIN: P(t) of a node from its slot of the window instead of the batch; nothing else differs.
template <typename T, int MODE, bool WIN = false>
__global__ void __launch_bounds__(PML_SIM_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) simulate_kernel(PmlSimArgs a) {
    static_assert(!WIN || MODE != PML_SIM_F81, "the window holds matrices");
    typedef SimWord<T> SW;
    typedef typename SW::W Word;
    extern __shared__ double sim_lds[];
    double* pcdf = sim_lds;
    const int k = a.k;
    const int tid = threadIdx.x;
    // cumulative pi, by wavefront 0 (the same sums in every workgroup)
    if (tid < 64) {
        double run = 0.0;
        for (int b0 = 0; b0 < k; b0 += 64) {
            const int b = b0 + tid;
            const double inc = sim_wave_scan(b < k ? a.pi[b] : 0.0, tid) + run;
            if (b < k) pcdf[b] = inc;
            run = __shfl(inc, 63, 64);
        }
    }
    __syncthreads();
    const double ptotal = pcdf[k - 1];
    double* tab = MODE == PML_SIM_MATRIX_LDS ? sim_lds + k
                                             : (MODE == PML_SIM_MATRIX_SCRATCH ? a.scratch + (size_t)blockIdx.x * k * k : nullptr);
    Word* states = reinterpret_cast<Word*>(a.states);
    const size_t rw = a.rs / 4;   // row stride in words
    const long long n_items = (long long)a.n_lists * a.n_tiles;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int li = (int)(item / a.n_tiles);
        const int tuple = (int)(item % a.n_tiles) * blockDim.x + tid;
        const bool active = tuple < a.n_tuples;
        const unsigned g0 = a.rep_offset + 4u * (unsigned)tuple;
        int q0, q1;
        if (a.lists != nullptr) {
            q0 = a.list_off[li];
            q1 = a.list_off[li + 1];
        } else {
            q0 = a.first_node + li;
            q1 = q0 + 1;
        }
        // a list's entry carries the ids the step needs, and the next entry is loaded a step ahead: the walk's dependent chain is
        // one load per node (the parent's states), not three (list -> parent -> states)
        int4 next = a.lists != nullptr ? a.lists[q0] : make_int4(0, 0, 0, 0);
        for (int q = q0; q < q1; ++q) {
            int n, p, slot;
            unsigned key, prow;
            if (a.lists != nullptr) {
                const int4 cur = next;
                if (q + 1 < q1) next = a.lists[q + 1];
                n = cur.x;
                key = (unsigned)cur.y;
                p = cur.z;
                prow = (unsigned)cur.z;
                slot = cur.w;
            } else {
                n = q;
                p = a.parent[n];
                key = (unsigned)(a.api_id ? a.api_id[n] : n);
                prow = p < 0 ? 0u : (unsigned)(a.api_id ? a.api_id[p] : p);
                slot = li;
            }
            if (MODE != PML_SIM_F81 && p >= 0) {
                // the branch's cumulative rows: row a (parent state) of P is column a of the stored transpose
                __syncthreads();   // (the previous node's draws are done with the table)
                const double* Pt = a.P + (size_t)(WIN ? slot : n) * k * a.ks;
                for (int r = tid; r < k; r += blockDim.x) {
                    double run = 0.0;
                    for (int b = 0; b < k; ++b) {
                        run += fmax(Pt[(size_t)b * a.ks + r], 0.0);
                        tab[r * k + b] = run;
                    }
                }
                __syncthreads();
            }
            if (!active) continue;
            unsigned x[4];
            sim_bits(a.seed, key, g0, x);
            int s[4];
            if (p < 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = sim_bisect(pcdf, k, sim_u(x[i]) * ptotal);
            } else {
                int ps[4];
                SW::unpack(states[(size_t)prow * rw + tuple], ps);
                if (MODE == PML_SIM_F81) {
                    const double e = a.E[n];
                    const double scale = e < 1.0 ? ptotal / (1.0 - e) : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double u = sim_u(x[i]);
                        s[i] = u < e ? ps[i] : sim_bisect(pcdf, k, (u - e) * scale);
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double* row = tab + ps[i] * k;
                        s[i] = sim_bisect(row, k, sim_u(x[i]) * row[k - 1]);
                    }
                }
            }
            states[(size_t)key * rw + tuple] = SW::pack(s);
        }
    }
}
