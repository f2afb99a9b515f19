// Ancestral scenarios drawn from the joint posterior of a column, on the device (pml_sample_scenarios).
//
// The law is the one marginal_counts samples (pastml/ml.py:786-824, pml_kernels_counts.h), applied per repetition instead of
// per count: a root draws from its marginal posterior row; a child n of a parent in state a draws b with probability
// proportional to
//     w_n[b] max(P_n[b][a], 0),      w_n[b] = BU_n[b] pi_b mask_n[b],  BU = 1 at tips.
// The masks are the ones the marginal pass ran with -- with tau == 0 those the zero-branch handling altered (ml.py:352-387):
// the scenarios follow that pass's law, and the fractional bookkeeping the reference keeps for altered pairs, which exists for
// the count table only, has no part here.  The lazy base-2 scale of a bottom-up row is common to the row and cancels.  If the
// weights of a (n, a) sum to zero the node draws from its own posterior row with the same uniform, and the draw is counted
// (n_fallback): a consistent pass produces none.
//
// Work, layout and draws are the forward simulator's (pml_kernels_simulate.h): items are (node list, repetition tile), a
// thread owns 4 consecutive repetitions, parents come before children inside a list, the rows [node][rep] are in the caller's
// numbering and a thread's parent read and child write are one 4-byte word (uint8, k <= 256) or 8 bytes (uint16).  One
// Philox-4x32-10 call keyed by seed, counter (global repetition / 4, caller's node id, 0, tag) gives the 4 uniforms of 4
// repetitions, u = x * 2^-32; the tag is this sampler's own.  The result is a pure function of (seed, node, global repetition).
//
//   F81 / JC / EFT: P is never formed.  P_n[b][a] = (1 - e) pi_a + [a = b] e, so the weights of parent state a are
//                   (1 - e) pi_a w[b] + [a = b] e w[a]: the workgroup builds ONE cumulative table of w_n per node (a wave scan,
//                   total S), and a draw decides between "stay at a" (u W_a < e w[a], W_a = (1 - e) pi_a S + e w[a]) and a
//                   bisection in that table.  O(k) table work per node.  A zero branch (e = 1) copies exactly.
//   HKY / JTT / CUSTOM_RATES: the workgroup builds the cumulative rows cdf[a][b] = sum_{b' <= b} w_n[b'] max(P_n[b'][a], 0) of a
//                   branch from the P(t) batch (row a of the stored transpose, summed left to right), in LDS up to
//                   PML_SIM_LDS_K states or in a per-workgroup slice of a scratch buffer, then every lane scales u by its row's
//                   sum and bisects.
// Every product that feeds a sum is rounded on its own (a statement each: no contraction into an FMA), so the arithmetic can
// be restated operation by operation (tests/scenario_ref.py).
#pragma once
#include "pml_kernels_simulate.h"

#define PML_SCEN_TAG 0x7363656eu   // word 3 of the counter (the simulator's: 0x73696d75, the counts sampler's: 0x51ed270b)

struct PmlScenArgs {
    const int* parent;        // internal ids
    const int* api_id;        // caller's id of an internal node (null: the same)
    const int* n_children;
    const int4* lists;        // as PmlSimArgs::lists (null: list i is the single node first_node + i)
    const int* list_off;      // [n_lists + 1]
    int first_node, n_lists;
    int n_tiles;              // repetition tiles per list (blockDim.x tuples each)
    int n_tuples;             // rs / 4
    int n_rep;                // repetitions asked for (the padding of the last tuple is drawn, not counted)
    size_t rs;                // row stride (elements)
    void* states;             // [N][rs], caller's numbering
    unsigned rep_offset;
    u64 seed;
    int k, ks, W;
    const double* pi;         // [ks] of the column; the per-node arrays below are the column's, in the library's numbering
    const u64* masks;         // [N][W]
    const double* bu;         // [N][ks] (tips: not stored)
    const double* post;       // [N][ks]
    const double* E;          // [N] (F81)
    const double* P;          // [N][k][ks] (matrix models): P^T per branch; WIN: the column's window [B][k][ks] (PmlSimArgs::P)
    double* scratch;          // [gridDim.x][k][k] (PML_SIM_MATRIX_SCRATCH)
    unsigned long long* n_fallback;
};

// the 4 uniforms (as 32-bit integers) of global repetitions g0 .. g0 + 3 of node `key`: word g & 3 of block g >> 2
__device__ __forceinline__ void scen_bits(u64 seed, unsigned key, unsigned g0, unsigned (&x)[4]) {
    unsigned a[4] = {g0 >> 2, key, 0u, PML_SCEN_TAG};
    philox4x32_10(a, (unsigned)seed, (unsigned)(seed >> 32));
    const unsigned sh = g0 & 3u;   // (launch-uniform: rep_offset % 4)
    if (sh == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = a[i];
        return;
    }
    unsigned b[4] = {(g0 >> 2) + 1u, key, 0u, PML_SCEN_TAG};
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

// w_n[b] of node row `row` of the column
__device__ __forceinline__ double scen_weight(const PmlScenArgs& a, size_t row, bool tip, int b) {
    const bool allowed = (a.masks[row * a.W + (b >> 6)] >> (b & 63)) & 1ull;
    if (!allowed) return 0.0;
    return tip ? a.pi[b] : a.bu[row * a.ks + b] * a.pi[b];
}

// a (n, a) without weight: the first b whose running sum of the node's posterior row exceeds u times the row's sum
// (the sums left to right; never taken after a consistent pass)
__device__ __forceinline__ int scen_fallback(const double* post, int k, double u) {
    double total = 0.0;
    for (int b = 0; b < k; ++b) total += post[b];
    const double w = u * total;
    double run = 0.0;
    for (int b = 0; b < k - 1; ++b) {
        run += post[b];
        if (run > w) return b;
    }
    return k - 1;
}

// Items (list, tile) in a grid-stride loop over blockIdx.x; all threads of a workgroup take the same item and build the
// node's table together.  Dynamic LDS, F81: pi [k], w_n [k], the cumulative table [k]; matrix models: w_n [k] (a root: its
// cumulative posterior), then (MATRIX_LDS) the rows [k][k].
// WIN: P(t) of a node from its slot of the window (the fourth field of a list entry; entry i of a level launch: i).
template <typename T, int MODE, bool WIN = false>
__global__ void __launch_bounds__(PML_SIM_THREADS) scenarios_kernel(PmlScenArgs a) {
    static_assert(!WIN || MODE != PML_SIM_F81, "the window holds matrices");
    typedef SimWord<T> SW;
    typedef typename SW::W Word;
    extern __shared__ double scen_lds[];
    const int k = a.k;
    const int tid = threadIdx.x;
    double* pil = scen_lds;                                              // (F81)
    double* wv = MODE == PML_SIM_F81 ? scen_lds + k : scen_lds;
    double* cdf = MODE == PML_SIM_F81 ? scen_lds + 2 * k : scen_lds;    // (matrix models: roots only)
    double* tab = MODE == PML_SIM_MATRIX_LDS ? scen_lds + k
                                             : (MODE == PML_SIM_MATRIX_SCRATCH ? a.scratch + (size_t)blockIdx.x * k * k : nullptr);
    if (MODE == PML_SIM_F81)
        for (int b = tid; b < k; b += blockDim.x) pil[b] = a.pi[b];   // (the first node's barrier covers it)
    Word* states = reinterpret_cast<Word*>(a.states);
    const size_t rw = a.rs / 4;   // row stride in words
    const long long n_items = (long long)a.n_lists * a.n_tiles;
    unsigned fallen = 0;
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
        int4 next = a.lists != nullptr ? a.lists[q0] : make_int4(0, 0, 0, 0);   // (loaded a step ahead, as in the simulator)
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
            const double* post = a.post + (size_t)n * a.ks;
            // the node's table (p and n are the same in every thread of the workgroup)
            __syncthreads();   // (the previous node's draws are done with the tables)
            if (p < 0 || MODE == PML_SIM_F81) {
                // wavefront 0: the cumulative posterior of a root / w_n and its cumulative table
                if (tid < 64) {
                    const bool tip = a.n_children[n] == 0;
                    double run = 0.0;
                    for (int b0 = 0; b0 < k; b0 += 64) {
                        const int b = b0 + tid;
                        double w = 0.0;
                        if (b < k) w = p < 0 ? post[b] : scen_weight(a, (size_t)n, tip, b);
                        const double inc = sim_wave_scan(w, tid) + run;
                        if (b < k) {
                            if (MODE == PML_SIM_F81) wv[b] = w;
                            cdf[b] = inc;
                        }
                        run = __shfl(inc, 63, 64);
                    }
                }
            } else {
                const bool tip = a.n_children[n] == 0;
                for (int b = tid; b < k; b += blockDim.x) wv[b] = scen_weight(a, (size_t)n, tip, b);
                __syncthreads();
                // row a (parent state) of the branch: P_n[b][a] is entry b of row a of the stored transpose
                const double* Pt = a.P + (size_t)(WIN ? slot : n) * k * a.ks;
                for (int r = tid; r < k; r += blockDim.x) {
                    double run = 0.0;
                    for (int b = 0; b < k; ++b) {
                        const double t = wv[b] * fmax(Pt[(size_t)r * a.ks + b], 0.0);
                        run += t;
                        tab[r * k + b] = run;
                    }
                }
            }
            __syncthreads();
            if (!active) continue;
            unsigned x[4];
            scen_bits(a.seed, key, g0, x);
            int s[4];
            if (p < 0) {
                const double total = cdf[k - 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] = sim_bisect(cdf, k, sim_u(x[i]) * total);
            } else {
                int ps[4];
                SW::unpack(states[(size_t)prow * rw + tuple], ps);
                if (MODE == PML_SIM_F81) {
                    const double e = a.E[n];
                    const double S = cdf[k - 1];
                    const double rest = (1.0 - e) * S;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double u = sim_u(x[i]);
                        const int pa = ps[i];
                        const double move = rest * pil[pa];   // (1 - e) pi_a S: the weight of a draw from the table
                        const double stay = e * wv[pa];
                        const double Wa = move + stay;
                        if (Wa > 0.0) {
                            const double t = u * Wa;
                            s[i] = t < stay ? pa : sim_bisect(cdf, k, (t - stay) * (S / move));
                        } else {
                            s[i] = scen_fallback(post, k, u);
                            fallen += 4 * tuple + i < a.n_rep;
                        }
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const double u = sim_u(x[i]);
                        const double* row = tab + ps[i] * k;
                        const double Wa = row[k - 1];
                        if (Wa > 0.0) {
                            s[i] = sim_bisect(row, k, u * Wa);
                        } else {
                            s[i] = scen_fallback(post, k, u);
                            fallen += 4 * tuple + i < a.n_rep;
                        }
                    }
                }
            }
            states[(size_t)key * rw + tuple] = SW::pack(s);
        }
    }
    if (fallen) atomicAdd(a.n_fallback, (unsigned long long)fallen);
}
