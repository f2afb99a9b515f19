// Horizontal merging of a vertically compressed forest (pastml/visualisation/tree_compressor.py: collapse_horizontally
// :164-211): siblings with equal configurations collapse into the first of them.  One pass = one call; integer work only.
//
// The configuration class of a vertex v is sig(v) = (bin[v], states(v), the set of (width[c], class(c)) over v's surviving
// children c), and it is labelled EXACTLY by hash-consing: a table of 64-bit keys (a << 32 | b) filled with atomicCAS, where
// the id of a pair is the slot that holds it.  cons(a, b) returns the same slot for the same pair and different slots for
// different pairs -- the hash only chooses where the probing starts, equality is that of the full key.  A sequence
// i1, i2, ..., in is labelled by the fold cons(... cons(cons(seed, i1), i2) ..., in); the seeds are no slot numbers (the table
// has at most 2^31 slots), so by induction two sequences get the same label iff they are equal, whatever their lengths.
//   states(v):  seed HZ_SEED_STATES, then the 32-bit halves of the W words of every column  -> sclass[v]  (one launch, all
//               vertices at once: it does not depend on the children)
//   sig(v):     seed HZ_NIL, then bin[v] (>= 0, so the key is never the empty marker), sclass[v], then (width, class) of the
//               surviving children SORTED by (width << 32 | class) -- the classes of a vertex's surviving children are pairwise
//               different, so the keys are, and the sorted sequence is a canonical form of the set.
// Slot numbers depend on the order in which the lanes arrive; which vertices get EQUAL numbers does not, and only that is used.
//
// Grouping the children of p by class: a second table keyed (p, class) whose slots carry min(rank << 32 | vertex) -- the first
// child in child order -- and the sum of the widths.  Both are integer atomics, order-independent.  The parent reads them one
// level later (hz_resolve): the group's first child survives with the summed width, the others leave and point to it.
//
// Levels are the depths of the compressed forest, deepest first; a level is one launch for the vertices with few children (a
// lane each, insertion sort in registers) and one for the others (a workgroup each: bitonic sort in LDS up to PML_HZ_TILE
// children, in a global scratch run of the next power of two beyond it -- any arity).  Every probe loop is bounded by the
// table size: a full table raises the error flag and the call fails, nothing spins.
#pragma once
#include "pml_device.h"

#define PML_HZ_THREADS 256
#define PML_HZ_TILE PML_HZ_SORT_TILE   // (pml_launch.h) children of one vertex that are sorted in LDS: 8 KB of keys
#define PML_HZ_SMALL 16      // children of one vertex that one lane sorts itself

#define HZ_EMPTY (~0ull)
#define HZ_NIL 0xFFFFFFFFu
#define HZ_SEED_STATES 0xFFFFFFFEu

typedef unsigned int u32;

struct HzTables {
    u64* keys;      // [mask + 1] pairs of the labelling, HZ_EMPTY where free
    u32 mask;
    u64* gkeys;     // [gmask + 1] (parent, class) of the sibling groups
    u64* gbest;     // min(rank << 32 | vertex) of a group, ~0 where none
    int* gwsum;     // sum of the widths of a group
    u32 gmask;
    int* error;     // set to 1 when a table is full
};

__device__ __forceinline__ u32 hz_mix(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (u32)k;
}

// The slot of the pair (a, b), inserted if new.  A slot goes from HZ_EMPTY to its key once and never changes again, so a
// stale read can only show HZ_EMPTY for a taken slot, and then the CAS returns what is there.  At most mask + 1 probes.
__device__ __forceinline__ u32 hz_cons(u64* keys, u32 mask, u32 a, u32 b, int* error) {
    const u64 key = ((u64)a << 32) | b;
    u32 slot = hz_mix(key) & mask;
    for (u32 probe = 0; probe <= mask; ++probe) {
        u64 cur = keys[slot];
        if (cur == key) return slot;
        if (cur == HZ_EMPTY) {
            cur = atomicCAS((unsigned long long*)&keys[slot], HZ_EMPTY, (unsigned long long)key);
            if (cur == HZ_EMPTY || cur == key) return slot;
        }
        slot = (slot + 1) & mask;
    }
    atomicExch(error, 1);
    return 0;   // (a valid slot: whatever follows stays in bounds, and the call fails on the flag)
}

// sclass[v] for every live vertex.  sets: [n_cols][V][W].
__global__ void __launch_bounds__(PML_HZ_THREADS)
hz_states_kernel(HzTables t, const u64* sets, const unsigned char* live, u32* sclass, int V, int W, int n_cols) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V || !live[v]) return;
    u32 id = HZ_SEED_STATES;
    for (int c = 0; c < n_cols; ++c) {
        const u64* row = sets + ((size_t)c * V + v) * W;
        for (int w = 0; w < W; ++w) {
            const u64 x = row[w];
            id = hz_cons(t.keys, t.mask, id, (u32)x, t.error);
            id = hz_cons(t.keys, t.mask, id, (u32)(x >> 32), t.error);
        }
    }
    sclass[v] = id;
}

struct HzVertices {
    const int* parent;        // [V] row of the vertex above, -1 for a root
    const int* rank;          // [V] rank among the siblings (child order)
    const int* bin;           // [V]
    const int* width_in;      // [V]
    const u32* sclass;        // [V]
    const int* child_off;     // [V + 1] children (live on entry) of a vertex in child_idx
    const int* child_idx;
    u32* cls;                 // [V] class of the vertex, once its level has run
    u32* slot_of;             // [V] slot of its sibling group
    int* width;               // [V] width out (starts as width_in)
    unsigned char* live;      // [V] live out (starts as live_in)
    int* into;                // [V] starts as the vertex itself
    int* groups;              // number of groups of two or more
};

// What the level of c left for it: true and the key (width << 32 | class) if c survives, else c leaves for its group's first.
__device__ __forceinline__ bool hz_resolve(const HzTables& t, const HzVertices& a, int c, u64* key) {
    const u32 s = a.slot_of[c];
    const int first = (int)(u32)t.gbest[s];
    if (first != c) {
        a.live[c] = 0;
        a.into[c] = first;
        return false;
    }
    const int w = t.gwsum[s];
    if (w != a.width_in[c]) {   // (widths are positive: a sum over two or more is larger than each)
        a.width[c] = w;
        atomicAdd(a.groups, 1);
    }
    *key = ((u64)(u32)w << 32) | a.cls[c];
    return true;
}

__device__ __forceinline__ u32 hz_sig_head(const HzTables& t, const HzVertices& a, int v) {
    u32 id = hz_cons(t.keys, t.mask, HZ_NIL, (u32)a.bin[v], t.error);
    return hz_cons(t.keys, t.mask, id, a.sclass[v], t.error);
}

__device__ __forceinline__ u32 hz_sig_child(const HzTables& t, u32 id, u64 key) {
    id = hz_cons(t.keys, t.mask, id, (u32)(key >> 32), t.error);
    return hz_cons(t.keys, t.mask, id, (u32)key, t.error);
}

// The class of v is known: enter it into the group of its siblings of that class.
__device__ __forceinline__ void hz_enter(const HzTables& t, const HzVertices& a, int v, u32 id) {
    a.cls[v] = id;
    const int p = a.parent[v];
    if (p < 0) return;   // roots never merge
    const u32 s = hz_cons(t.gkeys, t.gmask, (u32)p, id, t.error);
    atomicMin((unsigned long long*)&t.gbest[s], (unsigned long long)(((u64)(u32)a.rank[v] << 32) | (u32)v));
    atomicAdd(&t.gwsum[s], a.width_in[v]);
    a.slot_of[v] = s;
}

// A lane per vertex of the level with at most PML_HZ_SMALL children.
__global__ void __launch_bounds__(PML_HZ_THREADS)
hz_level_small_kernel(HzTables t, HzVertices a, const int* list, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int v = list[i];
    u64 keys[PML_HZ_SMALL];
    int m = 0;
    const int e0 = a.child_off[v], e1 = a.child_off[v + 1];
    for (int e = e0; e < e1 && m < PML_HZ_SMALL; ++e) {
        u64 key;
        if (!hz_resolve(t, a, a.child_idx[e], &key)) continue;
        int j = m++;
        for (; j > 0 && keys[j - 1] > key; --j) keys[j] = keys[j - 1];
        keys[j] = key;
    }
    u32 id = hz_sig_head(t, a, v);
    for (int j = 0; j < m; ++j) id = hz_sig_child(t, id, keys[j]);
    hz_enter(t, a, v, id);
}

// A workgroup per vertex of the level with more children.  scratch_off[i]: where the vertex's run of the global scratch
// begins (the next power of two from its child count on), -1 for a vertex whose children fit the LDS tile.
__global__ void __launch_bounds__(PML_HZ_THREADS)
hz_level_block_kernel(HzTables t, HzVertices a, const int* list, const long long* scratch_off, u64* scratch) {
    __shared__ u64 tile[PML_HZ_TILE];
    __shared__ int count;
    const int v = list[blockIdx.x];
    const long long off = scratch_off[blockIdx.x];
    u64* buf = off < 0 ? tile : scratch + off;
    const int e0 = a.child_off[v], e1 = a.child_off[v + 1];
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    for (int e = e0 + (int)threadIdx.x; e < e1; e += PML_HZ_THREADS) {
        u64 key;
        if (hz_resolve(t, a, a.child_idx[e], &key)) buf[atomicAdd(&count, 1)] = key;   // (count <= e1 - e0: within the run)
    }
    __syncthreads();
    const int m = count;
    int P = 1;
    while (P < m) P <<= 1;   // (P <= the power of two from e1 - e0 on: the size of the run, or PML_HZ_TILE)
    for (int i = m + (int)threadIdx.x; i < P; i += PML_HZ_THREADS) buf[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = (int)threadIdx.x; i < P; i += PML_HZ_THREADS) {
                const int l = i ^ j;
                if (l > i) {
                    const u64 x = buf[i], y = buf[l];
                    if ((x > y) == ((i & k) == 0)) {
                        buf[i] = y;
                        buf[l] = x;
                    }
                }
            }
            __syncthreads();
        }
    if (threadIdx.x == 0) {
        u32 id = hz_sig_head(t, a, v);
        for (int j = 0; j < m; ++j) id = hz_sig_child(t, id, buf[j]);
        hz_enter(t, a, v, id);
    }
}

// A vertex under one that left leaves too: one round of pointer jumping on copies.  After r rounds gone[v] is the OR over v
// and the 2^r - 1 vertices above it (up[] of a root is the root).
__global__ void hz_down_kernel(const int* up_in, const unsigned char* gone_in, int* up_out, unsigned char* gone_out, int V) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int u = up_in[v];
    gone_out[v] = gone_in[v] | gone_in[u];
    up_out[v] = up_in[u];
}

__global__ void hz_down_init_kernel(const int* parent, const unsigned char* live_in, const unsigned char* live, int* up,
                                    unsigned char* gone, int V) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int p = parent[v];
    up[v] = (p >= 0 && live_in[v]) ? p : v;
    gone[v] = !live[v];
}

__global__ void hz_down_finish_kernel(const unsigned char* gone, unsigned char* live, int V) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    live[v] = !gone[v];
}
