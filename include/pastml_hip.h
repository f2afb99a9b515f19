/*
 * pastml_hip.h -- C-ABI of libpastml_hip.so: the MI355X (gfx950) implementation of PastML's maximum-likelihood ACR
 * hot path.  Plain pointers and sizes only; the caller owns every host buffer, the library owns the device buffers
 * behind the opaque pml_ctx.  Every function returns a status (0 = PML_OK); pml_last_error() gives the message of the
 * last failure on the calling thread.  A ctx may be used from one thread at a time; different ctxs are independent
 * (each has its own HIP stream), which is how pastml.acr.acr()'s per-character thread pool (pastml/acr.py:226-231)
 * maps onto the device.
 *
 * The reference (evolbioinfo/pastml) is pure Python and has no FFI: each entry point below names the reference
 * function(s) whose arithmetic it replaces (paths relative to the reference repository).
 *
 * Layout conventions
 *   nodes     forest-wide level (breadth-first) order: roots are ids 0..n_roots-1, the children of a node are
 *             contiguous (first_child[n] .. first_child[n]+n_children[n]-1), every depth is a contiguous id range
 *   columns   the batch axis: one column = one character (with its own masks and model parameters); all columns of
 *             a ctx share the tree, the number of states k and the model kind
 *   masks     allowed-state bit sets, W = (k+63)/64 uint64 words per (column, node), bit s of word s/64 = state s
 *   vectors   double[k] per (column, node), column-major: index ((col * n_nodes + node) * k + state)
 *   scales    every likelihood vector v carries a base-2 exponent E (true value = v * 2^E); the *_sf outputs are
 *             converted to the reference's convention (base-10, true = v / 10^sf, pastml/ml.py:121,148)
 */
#ifndef PASTML_HIP_H
#define PASTML_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pml_ctx pml_ctx;

enum {
    PML_OK = 0,
    PML_ERR_INVALID = 1,      /* bad argument / call order */
    PML_ERR_HIP = 2,          /* HIP runtime failure (message has the HIP error string) */
    PML_ERR_UNSUPPORTED = 3,  /* e.g. k > 512 (F81 family), k > 256 (HKY / eigen models) */
    PML_ZERO_LIKELIHOOD = 4   /* pastml/ml.py:139-145: a parent/child pair has non-intersecting states */
};

enum { PML_MODEL_F81 = 0, PML_MODEL_HKY = 1, PML_MODEL_EIGEN = 2 };

/* what pml_download() can fetch (debug / tests / host-side state selection) */
enum {
    PML_BUF_BU = 0,          /* double[n_nodes][k]  bottom-up vectors of one column (tips: their masks as 0/1)      */
    PML_BUF_BU_SF = 1,       /* double[n_nodes]     their base-10 scale (reference BU_LH_SF convention)              */
    PML_BUF_TD = 2,          /* double[n_nodes][k]  top-down vectors of all nodes (pastml/ml.py:273-290)             */
    PML_BUF_TD_SF = 3,       /* double[n_nodes]                                                                        */
    PML_BUF_POSTERIOR = 4,   /* double[n_nodes][k]  marginal posteriors                                                */
    PML_BUF_LH_SUM = 5,      /* double[n_nodes]     sum of the (scaled) marginal likelihoods, in [1, 2)                */
    PML_BUF_LH_SF = 6,       /* double[n_nodes]     base-10 scale of the marginal likelihoods (reference LH_SF)        */
    PML_BUF_JOINT_TABLE = 7, /* int32[n_nodes][k]   argmax tables of the joint sweep (roots: undefined)               */
    PML_BUF_JOINT_STATE = 8, /* int32[n_nodes]                                                                          */
    PML_BUF_BRANCH_EXP = 9   /* double[n_nodes]     F81 family: e = exp(-mu t') per branch                             */
};

const char* pml_last_error(void);
int pml_version(void);
/* first 16 hex digits of the sha256 over the sources (everything under pastml_amd/csrc and this header) the library was compiled from --
 * pastml_amd/build.py hands it to the compiler and rebuilds when the sources in the tree give another one;
 * "unknown" for a build made by hand without -DPML_BUILD_DIGEST */
const char* pml_build_digest(void);
int pml_device_count(int* count);

/* ---- context ------------------------------------------------------------------------------------------------- */
int pml_ctx_create(int device, pml_ctx** out);
int pml_ctx_destroy(pml_ctx* ctx);
int pml_ctx_sync(pml_ctx* ctx);
/*
 * Options (set before pml_tree_upload).  PML_OPT_CHERRY_FUSION (default 1): in the F81-family marginal sweeps,
 * internal nodes whose children are all tips are recomputed in registers instead of being stored in HBM (their
 * vectors, like the top-down vectors of tips, are computed when pml_download asks for them).  With it, on large
 * forests and 17 <= k <= 64, nodes with two stored children that each carry two cherries of two tips run as two-level
 * units, and above them nodes take pairs of plain children over as stacked units: those children's
 * bottom-up vectors are not stored either, same rule for downloads.
 * PML_OPT_KEEP_TD (default 0, may be changed at any time): the F81-family top-down sweep works from the stored
 * posteriors of the level above (TD o BU = posterior * sum / pi) and does not write the top-down vectors themselves;
 * with this option it stores them too.  pml_download(PML_BUF_TD / PML_BUF_TD_SF) repeats the sweep with the stores on
 * when they are missing and fills in the vectors no sweep stores (tips, fused cherries).  The matrix models (HKY,
 * eigen) always store the vectors of internal nodes.
 * PML_OPT_EIGEN_FUSED (default 1, may be changed at any time): eigen-decomposed models with 16 <= k <= 32 run the fused
 * matrix-core sweeps (P(t) built and consumed in registers); 0 selects the sweeps that read materialised P(t) from HBM.
 * PML_OPT_EIGEN_JOINT_VALU (default 1, may be changed at any time): the JOINT sweep of eigen-decomposed models with
 * k <= 32 runs on the FP64 vector units (the default: faster than the matrix cores for this sweep);
 * 0 sends it to the kernels PML_OPT_EIGEN_FUSED selects -- kept as the cross-check of the default path.
 * PML_OPT_IMPLICIT_TIP_POSTERIORS (default 0, may be changed at any time; F81 family, k <= 64): the top-down sweep does
 * not write the posterior rows of observed tips -- unit vectors, a third of the sweep's traffic on a binary tree; they
 * are written when the table is read (pml_download*, posterior_out, pml_select_states, pml_marginal_counts) or before
 * the masks that define them change.  The sums / exponents of every node are written as always.
 */
enum { PML_OPT_CHERRY_FUSION = 1, PML_OPT_KEEP_TD = 2, PML_OPT_EIGEN_FUSED = 3, PML_OPT_EIGEN_JOINT_VALU = 4,
       PML_OPT_IMPLICIT_TIP_POSTERIORS = 5 };
int pml_ctx_set_option(pml_ctx* ctx, int option, int value);
/*
 * The switches of the schedules (tuning and test variants; DESIGN.md section 6a lists them).  Every ctx has its own set:
 * the defaults are the environment variables PASTML_HIP_<NAME> as they stand when the ctx is created, and this call
 * overrides one of them for this ctx -- name with or without the PASTML_HIP_ prefix; is_set = 0 returns the switch to
 * "not given" (the built-in default), otherwise value is what the environment variable would have held (for the NO_* /
 * on-off switches: value != 0 = on).  Switches that shape what pml_tree_upload / pml_chars_alloc build (NO_SUPER,
 * SUPER_MIN, STACK_MIN, NO_STACK, BLOCK_NODES, SMALL_MAX_NODES, NO_SHAPE_SORT, F81_R, ...) must be set before the tree
 * is uploaded (PML_ERR_INVALID afterwards); the others take effect with the next sweep (captured launch sequences are
 * dropped).  Unknown names are PML_ERR_INVALID.  There is no process-wide state: two contexts may run different schedules.
 */
int pml_ctx_set_tunable(pml_ctx* ctx, const char* name, int64_t value, int is_set);
/* bytes of device memory currently held by the ctx / free on its device */
int pml_ctx_memory(pml_ctx* ctx, uint64_t* held, uint64_t* device_free);
/*
 * What the F81-family sweeps of this context (tree uploaded, columns allocated) will run: *level_schedule = 1 if they
 * take the level schedule with two-level / stacked units (0: single launch, subtree blocks, plain levels, other models),
 * and the numbers of two-level and of stacked nodes in it.  For tools that model the sweeps' traffic (bench.py's byte
 * model is checked against this); the reference has no counterpart.
 */
int pml_schedule_info(pml_ctx* ctx, int32_t* level_schedule, int32_t* n_two_level, int32_t* n_stacked);
/*
 * Which of the schedules the marginal sweeps of the F81 family will take on this context (tree uploaded, columns
 * allocated; enqueue_bottom_up's own decision): the whole sweep in one launch (small forests), subtree blocks + the top
 * above them (mid-size forests; *n_blocks = their number), the level schedule with two-level / stacked units
 * (*n_absorbed: always 0 -- round 4's general two-level units for ragged trees lost their A/B twice and were removed in
 * round 6; the argument is kept for binary compatibility), plain level launches; PML_SCHEDULE_OTHER_MODEL for the matrix / eigen models.  For tests that compare schedules bit for bit: they
 * assert that the schedule under test is the one that runs.
 */
enum { PML_SCHEDULE_SINGLE_LAUNCH = 0, PML_SCHEDULE_BLOCKS = 1, PML_SCHEDULE_TWO_LEVEL = 2, PML_SCHEDULE_LEVELS = 3,
       PML_SCHEDULE_OTHER_MODEL = 4 };
int pml_sweep_schedule(pml_ctx* ctx, int32_t* kind, int32_t* n_blocks, int32_t* n_absorbed);
/*
 * The library's own node numbering.  The layout rules above leave the order of the sibling groups inside a depth to the
 * caller; pml_tree_upload renumbers the nodes of a ragged forest so that the sibling groups a level's units gather lie
 * next to each other in memory ("height order", pml_api.hip: the children of stored nodes by the nodes' fused height, the tips
 * of cherries by the height of the cherry's parent).  Every per-node array of this interface -- masks, tip ids, posteriors,
 * downloads, joint states, selections, the ids of a zero-likelihood report -- stays in the CALLER's numbering: the library
 * permutes rows on the way in and out (host side; whole-table outputs of a renumbered forest cost that pass).  This call
 * reports the numbering in use: new_of_old[caller's id] = the library's id (int32[n_nodes]; the identity for forests that are
 * in height order as given -- balanced trees are).  For tools that model the schedules (bench.py); PASTML_HIP_NO_HEIGHT_ORDER
 * keeps the caller's numbering.
 */
int pml_tree_order(pml_ctx* ctx, int32_t* new_of_old);

/* ---- tree (replaces the ete3 traversals of pastml/ml.py:109,269,449) ------------------------------------------ */
/*
 * bu_order        internal nodes sorted by height (1..n_bu_levels); bu_offsets[n_bu_levels+1] delimits the levels
 * td_parents      internal nodes sorted by depth; td_parent_offsets[n_td_levels+1] delimits them per depth
 * td_offsets      [n_td_levels+1] id range of every depth level
 * post_rank       rank of each node in the reference's processing order (trees in turn, post-order each); only used
 *                 to report the same (parent, child) pair as pastml/ml.py:139-145 when the likelihood is zero
 */
int pml_tree_upload(pml_ctx* ctx, int32_t n_nodes, int32_t n_roots,
                    const int32_t* parent, const int32_t* first_child, const int32_t* n_children, const double* dist,
                    int32_t n_bu_levels, const int32_t* bu_offsets, const int32_t* bu_order,
                    int32_t n_td_levels, const int32_t* td_offsets,
                    const int32_t* td_parent_offsets, const int32_t* td_parents,
                    const int32_t* post_rank);

/* ---- characters (replaces initialize_allowed_states, pastml/ml.py:293-318) ------------------------------------- */
int pml_chars_alloc(pml_ctx* ctx, int32_t n_cols, int32_t k);
/* masks[col_end-col_begin][n_nodes][W] */
int pml_masks_upload(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint64_t* masks);
/* fast path: internal nodes all ones, tip j (node id tip_ids[j]) one-hot at states[col][j], or all ones if < 0 */
int pml_masks_from_tip_states(pml_ctx* ctx, int32_t col_begin, int32_t col_end,
                              int32_t n_tips, const int32_t* tip_ids, const int32_t* states);
/*
 * Masks before zero-branch alteration (pastml/ml.py:352-387), needed only by the joint sweep to rewrite the argmax
 * tables of altered nodes (unalter_zero_node_joint_states, pastml/ml.py:408-428).  NULL clears them.
 */
int pml_masks_initial_upload(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint64_t* masks);

/* ---- model parameters (replaces Model.transform_t + get_Pij_t state, pastml/models/__init__.py:269) -------------- */
/* per column: pi[k]; scalars sf, tau, tau_factor (t' = (t + tau) * tau_factor * sf) */
int pml_model_set_f81(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi,
                      const double* sf, const double* tau, const double* tau_factor);
int pml_model_set_hky(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi, const double* kappa,
                      const double* sf, const double* tau, const double* tau_factor);
/* d[k], A[k][k], Ainv[k][k] (row-major) per column: pastml/models/generator.py:16-30.  k <= 256 (PML_ERR_UNSUPPORTED beyond).
 * 65 <= k <= 128: the sum sweeps keep one matrix in LDS, which a reversible model allows (generator.py:33-51 builds no other):
 * the call checks that Ainv is A transposed and rescaled (Ainv[m][j] = c_m A[j][m] pi[j], to 1e-8) and re-orthonormalises the
 * eigenvectors on the device (they come from a general solver, orthonormal to 1e-12); where the check fails -- an eigenvalue that
 * repeats, handed over with a non-orthogonal basis -- the sweeps read P(t) of every branch from HBM, as they do beyond 128 states. */
int pml_model_set_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi,
                        const double* d, const double* A, const double* Ainv,
                        const double* sf, const double* tau, const double* tau_factor);

/* ---- P(t) ---------------------------------------------------------------------------------------------------------- */
/*
 * P(t) of column col for n_t explicit branch lengths -> P_out[n_t][k][k] row-major.
 * Replaces Model.get_Pij_t: pastml/models/F81Model.py:28-46, HKYModel.py:44-82, CustomRatesModel.py:70-79 +
 * generator.py:54-65.
 */
int pml_pij(pml_ctx* ctx, int32_t col, int32_t n_t, const double* t, double* P_out);
/*
 * Materialises the per-branch transition data of every column on the device (F81 family: e = exp(-mu t') per
 * branch; HKY / eigen models: the full k x k matrix per branch).  The sweeps call it implicitly when the model or
 * the tree changed.  If P_out != NULL, additionally copies out P for every branch: P_out[n_cols][n_nodes][k][k].
 * It hands out per-branch data by definition: on a context with a window (pml_pij_window_set) it still allocates and fills the
 * batch of the whole tree, which then stays until the window is set again; so does pml_download of PML_BUF_TD / PML_BUF_TD_SF,
 * which fills in the top-down vectors of the nodes no sweep stores from P(t) of every branch.  Nothing else does.
 */
int pml_pij_batch(pml_ctx* ctx, double* P_out);
/*
 * Eigen models with 33 .. 256 states: the sweeps that read P(t) -- the joint sweep beyond 64 states, every sweep beyond 128 and
 * wherever the fused sweeps are switched off -- build it in a window of `branches` matrices per column instead of keeping
 * n_nodes of them: a level is cut into runs of parents whose children fit the window, and each run's launch follows one that
 * builds exactly those branches' matrices (pml_pij_window.h).  This is the reference's way -- a branch's matrix is built where
 * it is needed and dropped, pastml/models/CustomRatesModel.py:70-79, generator.py:54-65 --; every matrix is computed by the
 * instructions that compute it for the batch, so the sweeps leave the same bits.  branches = 0: off, the batch as before.
 * Allocates n_cols x branches x k x ks doubles (branches capped at n_nodes) and frees the batch if there is one.
 * PML_ERR_UNSUPPORTED for F81 / HKY contexts, for k <= 32 and under PASTML_HIP_NO_MFMA / _NO_PIJ_WIDE (the batch is then built by
 * another kernel, whose bits a window would not leave; set after the window, they take it away at the next sweep); PML_ERR_INVALID below the largest fan-out of the forest (the message
 * names it) and before the first model is set.
 * The entries that read P(t) outside the sweeps -- pml_marginal_counts(_altered), pml_expected_counts, pml_simulate_states,
 * pml_sample_scenarios -- read the window too, in runs: one launch builds exactly the branches the next launch of the entry reads,
 * for the columns of the call only (the sampled counts: the runs of the top-down sweep; the exact counts: whole pieces of 128 ids,
 * in a window of one piece per column of their own where the context's is smaller; the simulator and the sampler: runs of nodes of
 * a depth level, then groups of whole frontier subtrees, the frontier moving down where a subtree exceeds the window).  They leave
 * what they leave on a context without a window, allocate no term in n_nodes x k x k, and the context holds after the call what
 * it held before.  Only pml_pij_batch and the download of the top-down vectors (PML_BUF_TD / _SF) still materialise the whole
 * tree: they hand out per-branch data by definition, allocate the batch as on any other context, and it stays until the window is
 * set again -- pml_pij_window_info reports batch_bytes == 0 until one of the two is called.
 * PASTML_HIP_PIJ_WINDOW=<branches> does the same for every context it fits (raised to the fan-out, capped at n_nodes).
 */
int pml_pij_window_set(pml_ctx* ctx, long long branches);
/* What is allocated now: the window's branches (0: off) and bytes, and the bytes of the whole-tree batch (0: never allocated or freed). */
int pml_pij_window_info(pml_ctx* ctx, long long* branches, long long* window_bytes, long long* batch_bytes);

/* ---- sweeps --------------------------------------------------------------------------------------------------------- */
/*
 * Bottom-up (Felsenstein / Pupko) sweep over all columns: pastml/ml.py:82-148 (get_bottom_up_loglikelihood,
 * calc_node_bu_likelihood, rescale_log).  is_marginal != 0: sum over child states; == 0: max + argmax tables.
 * loglik_out[n_cols] = sum over the trees of the forest of ln L.
 * On PML_ZERO_LIKELIHOOD err_parent[col] / err_child[col] (node ids, -1 if the column is fine) name the pair the
 * reference would have raised PastMLLikelihoodError for.
 */
int pml_bottom_up(pml_ctx* ctx, int is_marginal, double* loglik_out, int32_t* err_parent, int32_t* err_child);
/*
 * pml_bottom_up in two halves: submit puts the sweep on the context's stream and returns at once, collect waits for it
 * and hands out what pml_bottom_up would have.  A host loop that serves several contexts (groups of characters with
 * different numbers of states, each with its own optimisers: the reference runs them one after the other,
 * pastml/acr.py:213-231) submits all their sweeps before it waits for any: the sweeps overlap on the device and with
 * the host work between them.  Between the two calls nothing else may be called on the context.
 * How the wait is done is the library's business: for short sweeps of at most 64 columns the last kernel raises a word in
 * pinned memory and the host spins on it (the runtime reports the end of a replayed launch sequence 10 - 14 us late);
 * everything else synchronises the stream (always with the switch NO_SPIN_WAIT).  The results are the same.
 */
int pml_bottom_up_submit(pml_ctx* ctx, int is_marginal);
/*
 * pml_bottom_up_submit for some of the columns: active[n_cols], 0 = the column sits this sweep out (NULL = all).  What
 * pml_bottom_up_collect returns for such a column is what the last sweep that computed it returned (ln L) and "no error";
 * its parameters and masks must be those of that sweep.  For the optimisers of a group of characters, most of which
 * are done long before the last one (the reference optimises one character at a time, pastml/acr.py:213-231).  The
 * next sweep or pass submitted in any other way computes every column again.  F81 family, marginal sweep; otherwise the
 * flags are ignored.
 */
int pml_bottom_up_submit_columns(pml_ctx* ctx, int is_marginal, const uint8_t* active);
int pml_bottom_up_collect(pml_ctx* ctx, int is_marginal, double* loglik_out, int32_t* err_parent, int32_t* err_child);
/*
 * Top-down sweep + marginal likelihoods + posteriors, fused: pastml/ml.py:240-290 (calculate_top_down_likelihood),
 * :431-465 (calculate_marginal_likelihoods), :486-502 (convert_likelihoods_to_probabilities).  Needs a preceding
 * marginal pml_bottom_up with the same masks.  Outputs are optional (NULL = keep on the device only):
 * posterior_out[n_cols][n_nodes][k], lh_sum_out / lh_sf_out[n_cols][n_nodes] such that
 * log10(lh_sum) - lh_sf is the node's total log10-likelihood (the invariant of pastml/ml.py:468-483).
 * F81 family, k <= 64: the posterior row of an observed tip (one allowed state) is the unit vector of its mask and depends on
 * nothing else.  It is written by the first top-down sweep after the masks were set and not rewritten while it provably stands
 * (nothing wrote the masks, reallocated the table, changed the model kind, an option or a tunable, no pass failed or wrote
 * NaNs there): sweeps after a change of the parameters alone skip those stores.  The table a caller sees is unchanged -- after
 * every sweep every row is in memory, bit for bit what a sweep that writes them all leaves.  PASTML_HIP_NO_KEEP_TIP_ROWS (a
 * tunable) makes every sweep write every row.
 */
int pml_top_down_marginals(pml_ctx* ctx, double* posterior_out, double* lh_sum_out, double* lh_sf_out);
/*
 * pml_bottom_up(marginal) + pml_top_down_marginals in one call: both sweeps are submitted before the host waits, so a
 * marginal pass costs one host round trip instead of two (what pastml/ml.py:700-707 does per tree in ml_acr).  Same
 * outputs and statuses as the two calls; on PML_ZERO_LIKELIHOOD the top-down results are invalid.  The observed tips'
 * posterior rows are kept across passes as pml_top_down_marginals says: a loop that re-sends parameters and calls this writes
 * them once; a pass that returns an error makes the next one write them all.
 */
int pml_marginal_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child,
                      double* posterior_out, double* lh_sum_out, double* lh_sf_out);
/*
 * Joint reconstruction after a joint pml_bottom_up: pastml/ml.py:598-622 (choose_ancestral_states_joint).
 * joint_state_out[n_cols][n_nodes].
 */
int pml_joint_backtrace(pml_ctx* ctx, int32_t* joint_state_out);
/* pml_bottom_up(joint) + pml_joint_backtrace in one call (one host round trip); outputs and statuses of the two */
int pml_joint_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child, int32_t* joint_state_out);

/*
 * State selection on the device after pml_top_down_marginals: method 0 = MAP (pastml/ml.py:577-595), 1 = MPPA
 * (pastml/ml.py:505-574).  lh_mask (optional, [n_cols][n_nodes][W]): masks multiplied into the marginal likelihoods
 * first, i.e. the '.initial' masks of the nodes altered by zero-branch handling and all ones elsewhere
 * (ml.py:541-542, 593-594).  force_joint (MPPA): the joint states of the last pml_joint_backtrace are always kept.
 * The selected masks REPLACE the columns' allowed-state masks on the device (ready for the restricted sweep) and are
 * copied to masks_out[n_cols][n_nodes][W] / n_states_out[n_cols][n_nodes] if not NULL.
 */
int pml_select_states(pml_ctx* ctx, int method, int force_joint, const uint64_t* lh_mask, uint64_t* masks_out,
                      int32_t* n_states_out);

/*
 * Expected numbers of state changes i -> j per scenario, estimated from n_repetitions ancestral scenarios drawn from
 * the marginal posterior of column col: the sampling scheme of pastml/ml.py:753-862 (marginal_counts) for forests
 * without nodes altered by the zero-branch handling (ml.py:352-387; with them: pml_marginal_counts_altered), with a counter-based
 * generator (Philox-4x32-10 keyed by seed): statistical, not bitwise, parity with the reference's numpy draws.
 * Needs pml_bottom_up (marginal) and pml_top_down_marginals first.  counts_out[k][k].
 * On a context with a P(t) window (pml_pij_window_set) the level launches are cut into the runs of the top-down sweep and read
 * the window, built for this column only: the same draws, no batch of the whole tree.
 */
int pml_marginal_counts(pml_ctx* ctx, int32_t col, int32_t n_repetitions, uint64_t seed, double* counts_out);
/*
 * The same for a forest with nodes altered by the zero-branch handling (altered[n_nodes], 1 = altered; pastml/ml.py:352-387).  The
 * scenarios are drawn as above.  A (parent, child) pair with an altered end does not enter the sums, and a parent of such a pair
 * keeps its diagonal correction: the reference gives those pairs fractional counts from the state counts of their two nodes
 * (ml.py:806-812, 840-853, 857-858), which the caller forms from what comes back -- sums_out[k][k]: the sums of the draws of all
 * other pairs, diagonal corrected for all other parents, NOT divided by n_repetitions; state_counts_out[n_nodes][k]: how often
 * each node was in each state; same_out[n_nodes][k]: for a parent of such a pair, its same-state draws over its other children
 * (rows of other nodes are zero).  pastml_amd.ml.marginal_counts is that caller.  Windowed contexts: as pml_marginal_counts.
 */
int pml_marginal_counts_altered(pml_ctx* ctx, int32_t col, int32_t n_repetitions, uint64_t seed, const uint8_t* altered,
                                double* sums_out, int32_t* state_counts_out, int32_t* same_out);

/*
 * The exact counterpart of pml_marginal_counts for the columns [col_begin, col_end): the limit of its estimate for
 * n_repetitions -> infinity, in closed form from the vectors of the marginal pass (needs pml_bottom_up (marginal) and
 * pml_top_down_marginals first, PML_ERR_INVALID otherwise).  Per column, in units "per scenario", with
 *   w_n[b] = BU_n[b] pi_b mask_n[b],  M_n[a][b] = w_n[b] P_n[b][a] / sum_b' w_n[b'] P_n[b'][a]      (pastml/ml.py:819-824)
 * and q_n = the marginal posterior of node n (the scheme draws the root from it, ml.py:794-798, and a child from q_parent . M_n,
 * which for a reversible model is the child's posterior):
 *   pair (p, n), neither end altered:  counts[a][b] += q_p[a] M_n[a][b],  same_p[a] += q_p[a] M_n[a][a]   (rows with q_p[a] == 0 unused)
 *   after the children of p:           counts[i][i] -= min(q_p[i], same_p[i])                              (ml.py:859-860)
 * altered ([n_nodes], 1 = altered by the zero-branch handling, ml.py:352-387; or NULL): the pairs with an altered end are left out
 * of counts_out, their parents keep their diagonal correction, and same_out carries those parents' same_p over their other
 * children (rows of other nodes are zero) -- the contract of pml_marginal_counts_altered, with the reference's rules for those
 * pairs (ml.py:806-812, 840-855: ps = to_initial(q_p) if p is altered else q_p, ci likewise, norm = ci / sum(ci), counts[i][:] +=
 * norm ps[i], same_p[i] += norm[i] ps[i]) left to the caller: pastml_amd.ml.expected_counts.
 * counts_out[n_cols][k][k]; same_out[n_cols][n_nodes][k] or NULL.  F81 family: k <= 512, the sum over the branches runs on the FP64
 * matrix cores; HKY / eigen models: k <= 256.  No atomics: the result does not depend on launch geometry, on the schedule
 * switches, on the library's numbering or on the column a character sits in -- nor on a P(t) window (pml_pij_window_set): the
 * branch pass then runs in runs of whole pieces of 128 ids behind the build of their matrices for the columns of the call (in a
 * window of one piece per column of the call's own where the context's holds fewer than 128 branches), pieces, partials and the
 * order of every sum untouched, and the batch of the whole tree is not allocated.
 */
int pml_expected_counts(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint8_t* altered, double* counts_out,
                        double* same_out);

/*
 * The exact gradient of ln L of the columns [col_begin, col_end) under the F81 family (F81, JC, EFT), from the vectors of the
 * marginal pass (needs pml_bottom_up (marginal) and pml_top_down_marginals first, PML_ERR_INVALID otherwise) -- no sweep, no
 * finite differences.  Per column, with mu = 1 / (1 - pi . pi), t'_n = (d_n + tau) tau_factor sf the transformed length of the
 * branch above the non-root node n, e_n = exp(-mu t'_n), v_n the bottom-up vector of n (a tip: its 0/1 mask), s_n = pi . v_n,
 * m_n[i] = (1 - e_n) s_n + e_n v_n[i] and q_p the marginal posterior of n's parent, for every non-root n with e_n < 1:
 *   A_n = sum_i q_p[i] / m_n[i],  B_n = sum_i q_p[i] v_n[i] / m_n[i]          (terms with q_p[i] == 0 are zero)
 *   h_n = -mu e_n (B_n - s_n A_n)  = d ln L / d t'_n,   T0 = sum_n h_n,   T1 = sum_n h_n t'_n
 *   E[m] = sum_n (1 - e_n) A_n v_n[m] + sum over the roots r of v_r[m] / (pi . v_r)
 *   d_rates_out[col][3] = { T1 / sf,  T0 tau_factor sf  (d / d tau at FIXED tau_factor),  T1 / tau_factor }
 *   d_pi_out[col][k]    = E[m] + 2 mu pi_m T1        (every pi_m treated as free; the dependence of mu on pi is included)
 *   n_flat_out[col]     = the number of branches whose e_n is exactly 1.0 as a double (t' = 0, or below 1e-16)
 * Such a flat branch adds nothing to T1 and E (its factors t' and 1 - e vanish), but its share of T0 cannot be recovered from
 * stored posteriors: the tau component of a column is valid only where its n_flat is 0.  The masks are those the marginal pass ran
 * with.  PML_ERR_UNSUPPORTED: a context of HKY or eigen models.  PML_ERR_INVALID: no marginal pass, k < 2, or a column whose
 * pi . pi >= 1 (mu infinite).  No atomics: the nodes are walked in the caller's numbering in pieces whose size depends on k only,
 * the partials are summed in piece order, and the result's bits do not depend on launch geometry, on the schedule switches, on the
 * library's numbering or on which other columns are in the call.  The results of the marginal pass stay as they are.
 */
int pml_loglik_gradient(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* d_rates_out, double* d_pi_out,
                        int32_t* n_flat_out);

/*
 * The exact expected dwell times and Markov jumps of the columns [col_begin, col_end) under the F81 family (F81, JC, EFT), taken
 * under the posterior over whole histories, from the vectors of the marginal pass (needs pml_bottom_up (marginal) and
 * pml_top_down_marginals first, PML_ERR_INVALID otherwise) -- no sweep, no sampling.  Where pml_expected_counts compares the two
 * ends of a branch, this counts events: a change undone on the same branch is counted twice here and not at all there.
 * In the notation of pml_loglik_gradient, with L_n = (d_n + tau) tau_factor the smoothed length of the branch above the non-root
 * node n, x_n = mu t'_n, e_n = exp(-x_n), S_n = pi . v_n, o_n[i] = q_p[i] / m_n[i] (0 where q_p[i] == 0), O_n = sum_i o_n[i] and
 *   g = (1 - e) / x,   c0 = 1 - 2 g + e,   c1 = g - e                                   (g = 1, c0 = c1 = 0 at x = 0)
 *   a_n[i] = pi_i O_n S_n c0 + o_n[i] S_n c1,     b_n[i] = pi_i O_n c1 + o_n[i] e_n
 *   times_out[col][s]        = sum_n L_n (a_n[s] + b_n[s] v_n[s])          (units of smoothed length; their sum is sum_n L_n)
 *   jumps_out[col][i][j]     = sum_n x_n pi_j (a_n[i] + b_n[i] v_n[j]) for i != j, 0 on the diagonal: the expected number of
 *                              jumps i -> j
 *   branch_jumps_out[col][n] = x_n sum_i (a_n[i] (1 - pi_i) + b_n[i] (S_n - pi_i v_n[i])): the expected number of jumps on the
 *                              branch above n, in the caller's numbering; 0 for a root
 * Every term is non-negative; a branch with t' = 0 adds nothing.  jumps_out and branch_jumps_out may be NULL: what is not asked
 * for is not computed (without jumps_out the call is one streaming pass), and times_out has the same bits either way.  The masks
 * are those the marginal pass ran with.  PML_ERR_UNSUPPORTED: a context of HKY or eigen models, or k > 512.  PML_ERR_INVALID: no
 * marginal pass, k < 2, or a column whose pi . pi >= 1 (mu infinite).  No atomics: the nodes are walked in the caller's numbering
 * in pieces whose size depends on k only, the partials are summed in piece order, and the bits of every output do not depend on
 * launch geometry, on the schedule switches, on the library's numbering, on which other columns are in the call or on how often
 * it is called.  The results of the marginal pass stay as they are.
 */
int pml_expected_history(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* times_out, double* jumps_out,
                         double* branch_jumps_out);

/*
 * The same quantities -- exact expected dwell times and Markov jumps under the posterior over whole histories -- for a context of
 * eigen-decomposed models (pml_model_set_eigen: JTT, CUSTOM_RATES, HKY handed over by its d, A, Ainv), 2 <= k <= 256, from the
 * vectors of the marginal pass (needs pml_bottom_up (marginal) and pml_top_down_marginals first, PML_ERR_INVALID otherwise) by the
 * eigenbasis integral of Minin & Suchard / Hobolth & Jensen -- no sweep, no sampling and no P(t): memory is O(N k), and a context
 * with a P(t) window keeps no batch.  Per column, d[k], A[k][k], Ainv[k][k] the doubles of pml_model_set_eigen, Q = A diag(d) Ainv,
 * t'_n = (dist_n + tau) tau_factor sf, L_n = t'_n / sf; for every non-root node n with parent p and t'_n > 0:
 *   v_n      bottom-up vector of n (a tip: its 0/1 mask; any scaling cancels)
 *   r_n    = Ainv v_n,   E_n = exp(d t'_n) elementwise,   m_n = A (E_n o r_n)   (= P(t'_n) v_n)
 *   o_n[a] = q_p[a] / m_n[a] (0 where q_p[a] == 0), q_p the marginal posterior of p,   l_n = A^T o_n
 *   Phi_cd(t) = integral_0^t exp(d_c u) exp(d_d (t - u)) du = t exp(d_d t) phi((d_c - d_d) t),  phi(z) = expm1(z) / z, phi(0) = 1
 *               (= (E[c] - E[d]) / (d_c - d_d) where |z| >= 0.5; below, the series of phi at |z| times the smaller exponential)
 *   X_n[c][d] = l_n[c] Phi_cd(t'_n) r_n[d],   W = sum_n X_n,   G = diag(d) - Ainv diag(Q_ii) A
 *   times_out[col][s]        = (1 / sf) sum_cd Ainv[c][s] W[c][d] A[s][d]   (units of smoothed length; their sum is sum_n L_n)
 *   jumps_out[col][i][j]     = Q_ij sum_cd Ainv[c][i] W[c][d] A[j][d]       (i != j; the diagonal exactly 0)
 *   branch_jumps_out[col][n] = sum_cd G[c][d] X_n[c][d]       (caller's numbering; a root and a branch with t' = 0: exactly 0)
 * A branch with t' = 0 adds nothing.  The sums are not sums of non-negative terms: an entry that rounding leaves below zero is
 * returned as 0.0.  Output shapes and the optional NULLs are those of pml_expected_history: what is not asked for is not computed,
 * and times_out has the same bits either way.  The masks are those the marginal pass ran with.
 * PML_ERR_UNSUPPORTED: an F81 context (pml_expected_history serves it), an HKY context (hand the model over as an eigen model),
 * k > 256.  PML_ERR_INVALID: no marginal pass, k < 2, a column whose sf is not finite and positive or whose d is not finite (the
 * message names the column; a sub-range call serves the others).  A refused call leaves the context as it was.
 * No atomics: the nodes are walked in the caller's numbering in pieces of 512 ids, the partials are summed in piece order, and the
 * bits of every output do not depend on launch geometry, on which other columns are in the call, on the column a character sits
 * in, on which outputs are asked for or on how often it is called.  They do follow the schedule switches, which change the bits
 * of the eigen sweeps' posteriors.  The results of the marginal pass stay as they are.
 */
int pml_expected_history_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, double* times_out, double* jumps_out,
                               double* branch_jumps_out);

/*
 * pml_expected_history per time interval, with the number of lineages in each state at every boundary: exact, F81 family, from
 * the vectors of the marginal pass (needs one, PML_ERR_INVALID otherwise).  Notation of pml_expected_history: x_n, L_n, S_n,
 * o_n, O_n, v_n, the stored e_n inside m_n.
 * Inputs: node_time[N], a time per node in the caller's numbering and in any unit (dates, root distances); a child must not be
 * earlier than its parent.  boundaries[M + 1], T_0 < ... < T_M: bin m is [T_m, T_{m+1}), the last bin also contains T_M.
 * Segments: a non-root node n with parent p and extent h = node_time[n] - node_time[p] > 0 has in every bin with
 * lo = max(T_m, time_p) < hi = min(T_{m+1}, time_n) one segment with the fractions
 *   s1 = (lo - time_p) / h,   w = (hi - lo) / h,   r = (time_n - hi) / h
 * each formed exactly so, as one quotient of one difference of the given doubles (never as s2 - s1: a sliver next to a node keeps
 * its digits).  A branch with h == 0 has smoothed length only: one segment s1 = 0, w = 1, r = 0 in the bin that contains time_n,
 * none if no bin does.  What lies outside [T_0, T_M] is not counted.
 * Per segment, with y = w x_n, (e_y, c0_y, c1_y) the e, c0, c1 of pml_expected_history at y (their series below 1),
 * A = -expm1(-s1 x_n), B = -expm1(-r x_n):
 *   C0  = w (c0_y + (A + B) c1_y + A B e_y)        multiplies pi_i O S
 *   C1a = w (1 - A) (c1_y + B e_y)                 multiplies o_i S
 *   C1b = w (1 - B) (c1_y + A e_y)                 multiplies pi_i O v_j
 *   Cee = w (1 - A) (1 - B) e_y                    multiplies o_i v_j
 *   a[i] = pi_i O S C0 + o_i S C1a,   b[i] = pi_i O C1b + o_i Cee
 *   times_out[col][m][s]    += L_n (a[s] + b[s] v_n[s])
 *   jumps_out[col][m][i][j] += x_n pi_j (a[i] + b[i] v_n[j])      (i != j; the diagonal is 0)
 * Every term is non-negative, C0 + C1a + C1b + Cee = w, and with s1 = r = 0, w = 1 they are c0, c1, c1, e of
 * pml_expected_history: the bins of a call that covers the tree sum to its outputs.
 * Lineages: at every boundary T_m, over the branches with time_p <= T_m < time_n, at s = (T_m - time_p) / h, with
 * A = -expm1(-s x), B = -expm1(-(1 - s) x), 1 - s formed as (time_n - T_m) / h:
 *   lineages_out[col][m][j] += (1-A)(1-B) o_j v_j + (1-A) B o_j S + A (1-B) pi_j O v_j + A B pi_j O S
 * the posterior of the state at that point of the branch, which sums over j to 1: sum_j lineages_out[col][m][j] is the number of
 * branches alive at T_m.
 * Outputs: times_out [cols][M][k]; jumps_out [cols][M][k][k] or NULL; lineages_out [cols][M + 1][k] or NULL.  What is NULL is
 * not computed and times_out has the same bits either way; an empty bin is exact zeros.
 * PML_ERR_UNSUPPORTED: a context of HKY or eigen models, k > 512, or M k^2 > 2^24 (PML_HIST_TIME_MAX_CELLS: every non-empty bin
 * leaves at least one k x k partial per column in the call's scratch, 128 MiB per column at the bound).  PML_ERR_INVALID: no
 * marginal pass, k < 2, a column whose pi . pi >= 1, M < 1, boundaries that are not strictly ascending, a child earlier than its
 * parent (the message names the node), a value that is not finite.  A refused call leaves the context and the results of the
 * marginal pass as they were.  No atomics: the segments are sorted by (bin, caller's id) and summed in pieces whose size depends
 * on k only and which never straddle two bins, so the bits of every output do not depend on launch geometry, on the schedule
 * switches, on the library's numbering, on which other columns are in the call or on how often it is called -- and a bin's rows
 * of times_out and jumps_out do not depend on the other bins.
 */
#define PML_HIST_TIME_MAX_CELLS (1 << 24)
int pml_history_through_time(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* node_time, const double* boundaries,
                             int32_t M, double* times_out, double* jumps_out, double* lineages_out);

/*
 * pml_history_through_time for a context of eigen-decomposed models (JTT, CUSTOM_RATES, HKY handed over by its d, A, Ainv),
 * 2 <= k <= 256: pml_expected_history_eigen per time interval, with the number of lineages in each state at every boundary,
 * from the vectors of the marginal pass (needs one, PML_ERR_INVALID otherwise).  Inputs, bins, segments (s1, w, r, and
 * u = (time_n - lo) / h, each one quotient of one difference), output shapes and the optional NULLs are those of
 * pml_history_through_time: what is NULL is not computed and times_out has the same bits either way.  Notation of
 * pml_expected_history_eigen: d, A, Ainv, t'_n = (dist_n + tau) tau_factor sf, r_n = Ainv v_n, l_n = A^T o_n, o_n = q_p / m_n.
 * The integral Phi_cd(t) = integral_0^t exp(d_c u) exp(d_d (t - u)) du, u measured from the parent, restricted to the segment
 * [s1 t', (s1 + w) t'], factorises exactly: Phi_cd^seg = exp(d_c s1 t') Phi_cd(w t') exp(d_d r t'), every exponent <= 0.  Per
 * segment, with y = w t':
 *   ls[c] = l_n[c] exp(d_c s1 t'),   Ey[c] = exp(d_c y),   rs[d] = r_n[d] exp(d_d r t')
 *   X_seg[c][d] = ls[c] Phi_cd(y) rs[d]        (Phi from y, d_c, d_d, Ey[c], Ey[d] as pml_expected_history_eigen forms it: the
 *                                              difference quotient where |(d_c - d_d) y| >= 0.5, the 15-term series of phi below)
 *   W_m = sum of X_seg over the segments of bin m
 *   times_out[col][m][s]    = (1 / sf) sum_cd Ainv[c][s] W_m[c][d] A[s][d]        (a row sums to the smoothed length in the bin)
 *   jumps_out[col][m][i][j] = Q_ij sum_cd Ainv[c][i] W_m[c][d] A[j][d]            (i != j; the diagonal exactly 0)
 * A branch with t' = 0 adds nothing to times_out or jumps_out.  A branch with h == 0 is one segment s1 = 0, w = 1, r = 0: ls, Ey,
 * rs are then l_n, E_n, r_n in bits.  The sums have mixed signs: an entry that rounding leaves below zero is returned as 0.0.  The
 * bins of a call that covers the tree sum to pml_expected_history_eigen's outputs; an empty bin is exact zeros.
 * Lineages: at every boundary T_m, over the branches with time_p <= T_m < time_n, with s = (T_m - time_p) / h and
 * u = (time_n - T_m) / h:
 *   lineages_out[col][m][j] += (sum_c Ainv[c][j] l_n[c] exp(d_c s t')) (sum_d A[j][d] r_n[d] exp(d_d u t'))
 * the posterior of the state at that point of the branch, which sums over j to 1.  Where t' = 0 the term is q_p[j], the formula at
 * P = I.  A row is clamped at 0 after its sum.
 * Refused in this order.  PML_ERR_INVALID: no model, a bad column range, a NULL node_time, boundaries or times_out.
 * PML_ERR_UNSUPPORTED: an F81 context (pml_history_through_time serves it), an HKY context (hand the model over as an eigen
 * model).  PML_ERR_INVALID: no marginal pass, k < 2.  PML_ERR_UNSUPPORTED: k > 256, M k^2 > PML_HIST_TIME_MAX_CELLS.
 * PML_ERR_INVALID: what the plan refuses (M < 1, boundaries that are not strictly ascending, a child earlier than its parent, a
 * value that is not finite), then a column whose sf is not finite and positive or whose d is not finite (the message names the
 * column; a sub-range call serves the others).  A refused call launches nothing and leaves the context and the results of the
 * marginal pass as they were.
 * Scratch, per column and in doubles, with N nodes, S segments (N - roots + one per boundary a branch crosses), ks = k padded:
 * 3 N ks + N for the branches' vectors, 3 S ks + S for the segments', k^2 per piece of 512 segments -- at least one per non-empty
 * bin, so at most (S / 512 + M) k^2 --, 2 M k^2 for W_m and its first product, and k per 512 flagged segments: O(N k) + O(S k) +
 * O((S / 512 + M) k^2).  It grows linearly with M through S and through the three M k^2 terms, which the bound on M k^2 holds
 * to 384 MiB per column.
 * No atomics: the segments are sorted by (bin, caller's id) and summed in pieces of 512 (tiles of 16 within a piece for the
 * lineages) that never straddle two bins, so the bits of every output do not depend on launch geometry, on which other columns
 * are in the call, on the column a character sits in, on which outputs are asked for or on how often it is called -- and a bin's
 * rows of times_out and jumps_out do not depend on the other bins.  They do follow the schedule switches, which change the bits of
 * the eigen sweeps' posteriors.
 */
int pml_history_through_time_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* node_time,
                                   const double* boundaries, int32_t M, double* times_out, double* jumps_out, double* lineages_out);

/*
 * Maximum parsimony of n_cols characters of k states (k <= 512) on the uploaded forest: the bottom-up pass
 * (pastml/parsimony.py:92-122) and, per bit of methods, ACCTRAN (:125-158), DOWNPASS (:161-210) and DELTRAN (:213-242, on
 * the DOWNPASS sets), each with the number of state changes its sets need (:360-380, summed over the trees) and the number
 * of nodes by size of their set (what parsimonious_acr's num_scenarios / unresolved nodes / states per node are made of,
 * :280-290).  Needs pml_tree_upload only -- no pml_chars_alloc, no model; the scratch of the call (at most 7 x
 * n_cols * n_nodes * W * 8 bytes; the columns are walked in chunks if that does not fit, PASTML_HIP_PARS_MAX_COLS bounds a
 * chunk) is released before it returns.  Integer arithmetic only: results do not depend on launch geometry, chunking or the
 * library's numbering.
 *   given          [n_cols][n_nodes][W]  annotated states as masks, caller's numbering; all-zero words = node not annotated
 *   sets_out       [n_methods][n_cols][n_nodes][W], the requested methods in the order ACCTRAN, DOWNPASS, DELTRAN
 *   steps_out      [n_methods][n_cols]
 *   size_hist_out  [n_methods][n_cols][k + 1]: nodes by number of states kept
 * pml_parsimony_info: kernel launches of the last call and the time of its passes (HIP events; without transfers).
 */
enum { PML_PARS_ACCTRAN = 1, PML_PARS_DOWNPASS = 2, PML_PARS_DELTRAN = 4 };
int pml_parsimony(pml_ctx* ctx, int32_t n_cols, int32_t k, const uint64_t* given, int methods, uint64_t* sets_out,
                  int64_t* steps_out, int64_t* size_hist_out);
int pml_parsimony_info(pml_ctx* ctx, int64_t* launches, double* passes_ms);

/*
 * Vertical collapse of the uploaded forest (pastml/visualisation/tree_compressor.py: collapse_vertically :251-298 with the
 * lists compress_tree :87-96 starts from; what the Pajek map of pajek_timing = VERTICAL shows, :34-51): a node whose state sets
 * equal its parent's in EVERY one of the n_cols columns belongs to its parent's vertex (roots never merge; an all-zero set
 * is the empty set, equal to another empty set).  Needs pml_tree_upload only -- no pml_chars_alloc, no model; the scratch of the
 * call (n_cols * n_nodes * W * 8 bytes for the sets -- the columns are walked in chunks if that does not fit,
 * PASTML_HIP_COMPRESS_MAX_COLS bounds a chunk -- plus 23 bytes per node: five int32 and three byte arrays) is released before it returns.  Integer arithmetic
 * only: results do not depend on launch geometry, chunking or the library's numbering.  Every array is in the CALLER's
 * numbering, and so are the node ids that top_out and parent_vertex_out hold.
 *   sets                 [n_cols][n_nodes][W]  state sets as masks (the layout of pml_parsimony; narrower columns zero-padded)
 *   is_polytomy          [n_nodes] or NULL     non-zero: an internal node that internal_inside_out does not count (:94)
 *   top_out              [n_nodes]  the first node (nearest to the root) of the node's vertex; top_out[n] == n starts a vertex
 *   tips_inside_out      [n_nodes]  at a vertex's first node: the tips of the vertex (itself included); 0 elsewhere
 *   internal_inside_out  [n_nodes]  the same for its internal nodes that are not flagged is_polytomy
 *   parent_vertex_out    [n_nodes]  at a vertex's first node: the first node of the vertex above, -1 for a root; -1 elsewhere
 * The first node of a vertex is found by pointer jumping, ceil(log2(deepest node)) rounds whatever the shape of the forest.
 * pml_compress_vertical_info: HIP-event times of the last call's passes (equality with the parent over all columns, the
 * pointer jumping, the counts; without transfers; taken only while pml_profile_enable is on, else 0) and its number of rounds.  PASTML_HIP_COMPRESS_PLAIN_ATOMICS: one atomic
 * per node in the counts instead of one per run of neighbouring lanes with the same vertex (for measurements).
 */
int pml_compress_vertical(pml_ctx* ctx, int32_t n_cols, int32_t W, const uint64_t* sets, const uint8_t* is_polytomy,
                          int32_t* top_out, int32_t* tips_inside_out, int32_t* internal_inside_out, int32_t* parent_vertex_out);
int pml_compress_vertical_info(pml_ctx* ctx, double* merged_ms, double* jump_ms, double* counts_ms, int32_t* rounds);

/*
 * One pass of the horizontal merging of a vertically compressed forest (pastml/visualisation/tree_compressor.py:
 * collapse_horizontally :164-211): among the live children of every vertex, those of one configuration class collapse into the
 * first of them in child order.  The class of a vertex is (bin, its state sets in all n_cols columns, the SET of (width, class)
 * of its surviving children) -- its own width is no part of it -- and is labelled exactly, level by level from the deepest
 * vertices up, by hash-consing integer pairs in a device table with 64-bit compare-and-swap: the hash chooses where to look,
 * equality is that of the full pair.  The table is sized before the pass from the numbers of vertices, columns and words (twice
 * the pairs a pass can make; 8 bytes a slot); a full table is an error, not a wait.  The ctx supplies the device and the stream;
 * the uploaded forest is not used, and the scratch of the call is released before it returns.  Integer arithmetic only: the
 * results do not depend on the launch geometry or on the order in which lanes reach the table.
 *   parent     [n_vertices]  row of the vertex above, -1 for a root (roots never merge); the parent of a live vertex is live
 *   rank       [n_vertices]  >= 0, child order among the siblings (any increasing key; distinct among siblings)
 *   bin        [n_vertices]  >= 0
 *   width_in   [n_vertices]  >= 1 where live
 *   live_in    [n_vertices]  non-zero: the vertex takes part; the others are passed over (into = itself, live = 0, width = width_in)
 *   sets       [n_cols][n_vertices][W]  state sets as masks, narrower columns zero-padded; W <= 8
 *   into_out   [n_vertices]  the row the vertex merged into, itself if it stays
 *   live_out   [n_vertices]  1 if the vertex is live afterwards: it did not merge into a sibling, nor did a vertex above it
 *   width_out  [n_vertices]  the sum of the widths of its group at a group's first vertex, width_in elsewhere
 *   groups_out               groups of two or more, or NULL
 * The children of a vertex are put in order by (width, class): a lane's insertion sort up to 16 children, a workgroup's
 * bitonic sort in LDS up to the tile that pml_compress_horizontal_info reports, in global scratch beyond it -- any arity.
 * pml_compress_horizontal_info: HIP-event times of the last call (labelling of the states, the level loop, the pass that takes
 * the vertices below a merged one out; without transfers; taken only while pml_profile_enable is on, else 0), its levels (depths
 * of the vertex forest), kernel launches (at most two per level, plus 3 + ceil(log2(levels))), table slots, and the LDS tile.
 */
int pml_compress_horizontal(pml_ctx* ctx, int32_t n_vertices, int32_t n_cols, int32_t W, const int32_t* parent, const int32_t* rank,
                            const int32_t* bin, const int32_t* width_in, const uint8_t* live_in, const uint64_t* sets,
                            int32_t* into_out, uint8_t* live_out, int32_t* width_out, int32_t* groups_out);
int pml_compress_horizontal_info(pml_ctx* ctx, double* states_ms, double* levels_ms, double* down_ms, int32_t* levels,
                                 int64_t* launches, int64_t* table_slots, int32_t* sort_tile);

/*
 * The trimming of a horizontally merged forest (pastml/visualisation/tree_compressor.py: compress_tree :118-159,
 * remove_small_tips :214-248, remove_mediators :301-340) over its live vertices, entries in Pajek pre-order; the trees of the
 * forest side by side, each with a threshold of its own.  The ctx supplies the device and the stream; the uploaded forest is
 * not used, and the scratch of the call is released before it returns.  Integer and exactly rounded float64 work only: the
 * results do not depend on the launch geometry.
 *   parent        [n_vertices]  entry above, -1 for a root; parent[i] < i, and every subtree is a run of consecutive entries
 *   tree          [n_vertices]  in [0, n_trees), that of the parent
 *   n_tips_total  [n_vertices]  >= 0, tips inside over all configurations of the vertex
 *   width         [n_vertices]  >= 1, configurations merged into the vertex
 *   sets          [n_cols][n_vertices][W]  state sets as masks, narrower columns zero-padded; W <= 8
 *   trim_tree     [n_trees]     non-zero: the tree is over the gate (more than tip_size_threshold leaf vertices)
 *   tsize_out     [n_vertices]  (n_tips_total / width) * the product of the widths from the root down; 0 outside trim_tree.  A
 *                               product or a size of 2^53 or more fails the call (PML_ERR_UNSUPPORTED)
 *   threshold_out [n_trees]     the tip_size_threshold-th largest tsize among the non-root vertices with tsize > that of all
 *                               their children; NaN where nothing happens to the tree (not in trim_tree, or no candidate is smaller)
 *   keep_out      [n_vertices]  1: a root, or some vertex of its subtree has tsize >= threshold (1 outside the trimmed trees)
 *   spliced_out   [n_vertices]  1: a mediator that is spliced out -- kept, no root, width 1, no tips, one kept child, and in every
 *                               column at least two states that are exactly those of its parent and of its child after the
 *                               splices below it
 *   new_parent_out[n_vertices]  the nearest entry above that is not spliced out; -1 for a root and for a vertex that is gone
 *   moved_out     [n_vertices]  1: new_parent is not parent (the vertex goes behind the children that stayed)
 * The k-th largest candidate of every tree is taken on the host inside the call, from one download of the candidate values.
 * pml_compress_trim_info: HIP-event times of the last call (sizes and candidates, removal, mediators and parents; without
 * transfers; taken only while pml_profile_enable is on, else 0), the levels of the vertex forest, the rounds of the multiplier
 * (ceil(log2(levels))), kernel launches (0 where no tree is in trim_tree, 3 + rounds where none gets a threshold, else
 * 9 + rounds), and the entries of one workgroup of the prefix count.
 */
int pml_compress_trim(pml_ctx* ctx, int32_t n_vertices, int32_t n_cols, int32_t W, const int32_t* parent, const int32_t* tree,
                      const int32_t* n_tips_total, const int32_t* width, const uint64_t* sets, int32_t tip_size_threshold,
                      int32_t n_trees, const uint8_t* trim_tree, double* tsize_out, uint8_t* keep_out, uint8_t* spliced_out,
                      int32_t* new_parent_out, uint8_t* moved_out, double* threshold_out);
int pml_compress_trim_info(pml_ctx* ctx, double* sizes_ms, double* removal_ms, double* mediators_ms, int32_t* levels, int32_t* rounds,
                           int64_t* launches, int32_t* scan_tile);

/*
 * The timeline of the compressed map (pastml/tree.py: annotate_dates :51-65; pastml/visualisation/cytoscape_manager.py: the
 * get_date of visualize :751-762 and the milestone loop of _forest2json_compressed :219-268) over a forest given as arrays.
 * The ctx supplies the device and the stream; the uploaded forest is not used, and the scratch of the call is released before
 * it returns.  One addition per date in the order of the reference, minima and integer work: the results do not depend on the
 * launch geometry.  Node ids are breadth-first over the forest: level d is the run [level_offsets[d], level_offsets[d + 1]),
 * level 0 the roots, and the parent of a node of level d lies in level d - 1.
 *   level_offsets [n_levels + 1]  ascending from 0 to n_nodes
 *   parent        [n_nodes]   -1 for the roots
 *   dist          [n_nodes]   branch length above the node
 *   given         [n_nodes]   the date given for the node, NaN for none
 *   root_dates    [roots]     the date of a root without a given date
 *   alive         [n_nodes]   non-zero: the node is in the full tree after the trimming
 *   up            [n_nodes]   its nearest alive ancestor, -1 for a root; up[n] < n
 *   config        [n_nodes]   the configuration the node is inside, -1 for none
 *   is_tip, is_polytomy [n_nodes]   the original tips; the nodes that are counted in no configuration
 *   top           [n_configs] the first node of every configuration
 *   below_lo, below_hi [n_configs]  the tips below top are tip_order[below_lo : below_hi]
 *   tip_order     [n_tips]    the tips in left-to-right leaf order
 *   member_offsets[n_vertices + 1]  the configurations of vertex v are the run [member_offsets[v], member_offsets[v + 1])
 *   timeline_type 0 SAMPLED, 1 NODES, 2 LTT
 *   milestones    [n_milestones]  strictly ascending, at most 64
 *   dates_only    non-zero: return after the dates (date_out is filled, nothing else is read or written but the first five
 *                 node arrays), so that the caller can choose the milestones
 * Results: date_out, get_date_out [n_nodes]; n_roots .. below_max [n_vertices][n_milestones] -- the configurations of the vertex
 * whose top has get_date <= milestone i, and the minimum and maximum over them of the tips inside, the internal nodes inside and
 * the tips below at that milestone (0 where there is none); first_milestone [n_vertices], n_milestones for never.
 * pml_timeline_info: HIP-event times of the last call (dates, get_date, bins, role counts, tips below, vertices; without
 * transfers; taken only while pml_profile_enable is on, else 0), the levels, the kernel launches, the launches of the date sweep
 * (a level of more than fuse_width nodes is a launch of its own, a run of consecutive smaller levels is one launch of one
 * workgroup) and fuse_width.
 */
typedef struct pml_timeline_in {
    int32_t n_nodes, n_levels, n_configs, n_tips, n_vertices, timeline_type, n_milestones, dates_only;
    const int32_t* level_offsets;
    const int32_t* parent;
    const double* dist;
    const double* given;
    const double* root_dates;
    const uint8_t* alive;
    const int32_t* up;
    const int32_t* config;
    const uint8_t* is_tip;
    const uint8_t* is_polytomy;
    const int32_t* top;
    const int32_t* below_lo;
    const int32_t* below_hi;
    const int32_t* tip_order;
    const int32_t* member_offsets;
    const double* milestones;
} pml_timeline_in;
typedef struct pml_timeline_out {
    double* date;
    double* get_date;
    int32_t* n_roots;
    int32_t* tips_min;
    int32_t* tips_max;
    int32_t* internal_min;
    int32_t* internal_max;
    int32_t* below_min;
    int32_t* below_max;
    int32_t* first_milestone;
} pml_timeline_out;
int pml_timeline(pml_ctx* ctx, const pml_timeline_in* in, const pml_timeline_out* out);
int pml_timeline_info(pml_ctx* ctx, double* stage_ms /* [6] */, int32_t* levels, int64_t* launches, int64_t* date_launches,
                      int32_t* fuse_width);

/*
 * n_repetitions scenarios of column col drawn forward from the roots (pastml/utilities/state_simulator.py:6-31):
 * roots ~ pi, child ~ row (parent state) of P_n(t).  Draws keyed by (seed, caller's node id, rep_offset + r):
 * results do not depend on launch geometry, chunking or the library's internal numbering.
 * states_out[n_nodes][n_repetitions], caller's numbering; uint8 for k <= 256, else uint16.
 * Needs a model (pml_model_set_*), no sweep.
 * On a context with a P(t) window (pml_pij_window_set) the depth levels above the frontier run in runs of at most `branches`
 * nodes and the frontier's subtrees in groups of whole subtrees of at most `branches` nodes together, each behind the build of
 * its matrices for this column; a frontier subtree larger than the window moves the frontier down for the call.  The same
 * states, more launches, no batch of the whole tree.
 */
int pml_simulate_states(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed,
                        void* states_out);

/*
 * n_repetitions scenarios of column col drawn from the joint posterior given the tips: complete, internally consistent
 * histories, one state per node and repetition.  The law is the one pml_marginal_counts samples (pastml/ml.py:786-824), applied
 * per repetition: a root draws from its marginal posterior row; a child n of a parent in state a draws b with probability
 * proportional to w_n[b] max(P_n[b][a], 0),  w_n[b] = BU_n[b] pi_b mask_n[b]  (BU = 1 at tips).  The masks are the ones the
 * marginal pass ran with: with tau == 0 those altered by the zero-branch handling (ml.py:352-387) -- the scenarios follow that
 * pass's law; the reference's fractional counts for altered pairs belong to the count table and have no part here.
 * Needs pml_bottom_up (marginal) and pml_top_down_marginals first, PML_ERR_INVALID otherwise.  F81 family: k <= 512, one
 * cumulative table per node; HKY / eigen models: k <= 256, cumulative rows per branch from the P(t) batch; PML_ERR_UNSUPPORTED
 * beyond.  Draws keyed by (seed, caller's node id, rep_offset + r) with a counter tag of their own: results do not depend on
 * launch geometry, chunking or the library's internal numbering, and calls with consecutive rep_offsets make up one larger call.
 * states_out[n_nodes][n_repetitions], caller's numbering; uint8 for k <= 256, else uint16.
 * n_fallback_out: the draws whose weights summed to zero and were taken from the node's own posterior row instead (with the
 * same uniform); 0 after a consistent pass.
 * On a context with a P(t) window: the windowed schedule of pml_simulate_states, the same states and the same count.
 */
int pml_sample_scenarios(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed,
                         void* states_out, int64_t* n_fallback_out);

/*
 * Stochastic character maps: n_repetitions whole histories of column col under the F81 family (F81, JC, EFT; k <= 512), drawn
 * on the device.  Where pml_expected_history gives the posterior means of the dwell times and of the Markov jumps, this gives
 * draws of them, for credible intervals.  The call draws the scenarios of pml_sample_scenarios (the same seed, the same bits;
 * they stay on the device unless states_out asks for them) and then, for every branch, a history between its two end states.
 * Q = mu (1 pi^T - I) is a Poisson process of rate mu whose events redraw the state from pi, so no rejection, no
 * uniformisation bound and no matrix is needed.  In the notation of pml_expected_history -- L_n = (d_n + tau) tau_factor,
 * x_n = mu t'_n, e_n the stored exp(-x_n) of the marginal pass -- for repetition g = rep_offset + r and a non-root node n whose
 * parent is in state a and which is in state b:
 *   1. the number of redraw events M.  x_n == 0: M = 0.  Otherwise q = 1.0 - e_n and u = draw 0.  a != b: target = u q.
 *      a == b: Wa = q pi[a] + e_n, t = u Wa; t < e_n: M = 0; else target = (t - e_n) / pi[a].  M >= 1 by inversion over the terms
 *      e x^m / m! (a zero-truncated Poisson):
 *          term = e_n x_n; cum = term; m = 1
 *          while cum <= target:  m += 1;  term = (term x_n) / m;  if cum + term == cum or m == 4096: stop;  cum += term
 *          M = m
 *   2. the spacings.  M >= 1: draws 1 .. M + 1 give w_i = -log((X_i + 0.5) 2^-32), i = 0 .. M (X the 32-bit word), Wsum their
 *      sum left to right, dwell_i = (L_n w_i) / Wsum (normalised exponentials: the spacings of M uniform order statistics).
 *      M = 0: the whole L_n is spent in a, no draw.
 *   3. the states.  s_0 = a, s_M = b; draws M + 2 .. 2 M give s_1 .. s_{M-1}, each the bisection of the cumulative table of pi
 *      (the one pml_simulate_states draws a root from) at u times its last entry, u = X 2^-32.  Interval i adds dwell_i to
 *      times_out[r][s_i]; every i >= 1 with s_{i-1} != s_i adds 1 to jumps_out[r][s_{i-1}][s_i] and to branch_jumps_out[n][r].
 *      Virtual events, which redraw the state they find, count nowhere.
 * Draw d of (n, g) is word d & 3 of Philox-4x32-10 keyed by the seed with the counter (g, caller's id of n, d >> 2, a tag of this
 * sampler's own); u = X 2^-32.  Every operation is rounded on its own.  The result is a pure function of (seed, node, global
 * repetition): launch geometry, chunking and the library's numbering never show, and calls with consecutive rep_offsets make
 * up one larger call.
 *   states_out       [n_nodes][n_repetitions] as pml_sample_scenarios writes them, or NULL
 *   times_out        [n_repetitions][k], units of smoothed branch length; a row sums to sum_n L_n
 *   jumps_out        [n_repetitions][k][k] or NULL: the number of jumps i -> j, zero diagonal
 *   branch_jumps_out [n_nodes][n_repetitions], caller's numbering, or NULL: the jumps on the branch above n; 0 for a root
 *   n_fallback_out   as pml_sample_scenarios
 * What is not asked for is not computed, and times_out has the same bits either way: no floating-point atomics -- the nodes are
 * walked in the caller's numbering in pieces whose size depends on n_nodes only, one thread adds the dwells of a repetition in
 * node order, and the pieces are summed in piece order.  The results of the marginal pass stay as they are.
 * PML_ERR_INVALID: no marginal pml_bottom_up and pml_top_down_marginals before, k < 2, pi . pi >= 1.  PML_ERR_UNSUPPORTED: a
 * context of HKY or eigen models, k > 512, or a branch with x_n > 512 (beyond it e_n leaves the normal doubles and the inversion
 * loses its meaning: such branches are not drawn, and the message carries their number).
 */
int pml_sample_histories(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed,
                         void* states_out, double* times_out, uint32_t* jumps_out, uint16_t* branch_jumps_out,
                         int64_t* n_fallback_out);

/*
 * pml_sample_histories per time interval: the sampled counterpart of pml_history_through_time, for credible intervals of the
 * rate i -> j in a period and of the number of lineages in a state at a date.  Repetition g = rep_offset + r of node n has
 * exactly the history pml_sample_histories draws for the same seed -- the same scenarios, the same draws (the same Philox counter),
 * the same event count M, exponentials w_0 .. w_M, Wsum and states s_0 = a, .., s_M = b.  New is only where on the branch the
 * events lie and how the history is cut at the boundaries.  node_time, boundaries, M and the bins are those of
 * pml_history_through_time, and so are the segments of a branch: s1, w, the flag `starts` (the branch is alive at the boundary
 * the bin begins with) and the zero-width point segments of the pseudo-bin M at T_M.
 *   Positions.  c_0 = 0; P_i = w_0 + .. + w_{i-1}, summed left to right, and c_i = P_i / Wsum for i = 1 .. M; c_{M+1} = 1, set and
 *      not computed.  History interval i is [c_i, c_{i+1}) in state s_i; event i >= 1 happens at c_i.
 *   Upper ends.  s2 of a segment is the s1 of the same branch's segment in the next bin (for a branch that leaves the range: of its
 *      point segment at T_M) -- the same quotient (T_{m+1} - time_p) / h, hence the same double; never s1 + w or 1 - r.  Where
 *      the branch ends inside the bin (every branch with h == 0 as well) s2 = 1 with the end included.  The segments of a branch
 *      tile it without gap or overlap, in bits: a position c belongs to the one segment with s1 <= c < s2 (<= 1 for the last).
 *      What lies outside [T_0, T_M] counts nowhere.
 *   Dwell.  Interval i gives segment (n, m) the time L_n w -- the segment's own w: a sliver keeps its digits, and a branch
 *      without events gives L_n w with no draw beyond draw 0 -- if c_i <= s1 and s2 <= c_{i+1}; otherwise lo = max(c_i, s1),
 *      hi = min(c_{i+1}, s2), v = hi - lo and, where v > 0, the time L_n v.  It is added to times_out[r][m][s_i].
 *   Jumps.  Event i >= 1 with s_{i-1} != s_i whose position belongs to segment (n, m) adds 1 to jumps_out[r][m][s_{i-1}][s_i].
 *      Virtual events count nowhere.
 *   Lineages.  Every segment with `starts`, those of the pseudo-bin M included, adds 1 to lineages_out[r][m][s_i] for the largest
 *      i with c_i <= s1: an event exactly at the boundary has already happened, and a branch that begins at the boundary
 *      (s1 == 0) shows its parent's state.  sum_j lineages_out[r][m][j] is the number of branches alive at T_m.
 * Every operation is rounded on its own.  With bins that cover the tree, the jumps of a repetition sum over the bins to
 * pml_sample_histories' exactly and its times to rounding.
 *   states_out     [n_nodes][n_repetitions] as pml_sample_scenarios writes them, or NULL
 *   times_out      [n_repetitions][M][k], units of smoothed branch length
 *   jumps_out      [n_repetitions][M][k][k] or NULL, zero diagonal
 *   lineages_out   [n_repetitions][M + 1][k] or NULL
 *   n_fallback_out as pml_sample_scenarios
 * What is NULL is not computed, and times_out has the same bits either way.  No floating-point atomics: the segments are sorted
 * by (bin, caller's id) and cut into pieces whose size depends on n_nodes only and which never straddle two bins; one thread adds
 * the dwells of a repetition in segment order and the pieces of a bin are summed in piece order.  The bits of every output are a
 * pure function of (seed, node, global repetition, the times, the boundaries): launch geometry, the schedule switches, the
 * library's numbering and chunking never show, calls with consecutive rep_offsets make up one larger call, and the rows of a bin
 * do not depend on the other bins.  The generator is counter-based: a branch that spans B bins is derived B times.  The results
 * of the marginal pass stay as they are.
 * PML_ERR_INVALID: what pml_sample_histories and pml_history_through_time answer with it (no marginal pass, k < 2, pi . pi >= 1;
 * M < 1, boundaries that are not strictly ascending, a child earlier than its parent -- the message names the node --, a value
 * that is not finite).  PML_ERR_UNSUPPORTED: a context of HKY or eigen models, k > 512, M k^2 > PML_HIST_TIME_MAX_CELLS, or a
 * branch with x_n > 512 (not drawn; the message carries their number, over the whole forest).  A refused call leaves the context
 * answering.
 */
int pml_sample_histories_through_time(pml_ctx* ctx, int32_t col, int32_t n_repetitions, int32_t rep_offset, uint64_t seed,
                                      const double* node_time, const double* boundaries, int32_t M, void* states_out,
                                      double* times_out, uint32_t* jumps_out, uint32_t* lineages_out, int64_t* n_fallback_out);

/* ---- multi-GPU (one process per GPU) ----------------------------------------------------------------------------------- */
/*
 * The characters of a run are independent (pastml/acr.py:213-231 hands them to a pool one by one, each with its own
 * model instance), so they shard over the GPUs of a node with the tree replicated and no exchange on the data path.
 * The one collective is the sum of the per-rank log-likelihoods (what a caller optimising shared parameters over all
 * characters, or reporting the total, needs): an all-reduce of 8 bytes over RCCL / xGMI on the ctx's own stream.
 * librccl is opened with dlopen on first use.  Rank 0 makes the id with pml_comm_unique_id and the host hands it to the
 * other ranks (file, socket, environment: 128 opaque bytes); every rank then calls pml_comm_init on its ctx (collective).
 * world == 1 needs neither an id nor librccl.  The communicator survives pml_tree_upload and dies with the ctx.
 */
#define PML_COMM_ID_BYTES 128
enum { PML_COMM_SUM = 0, PML_COMM_MAX = 1 };
int pml_comm_unique_id(unsigned char* id_out /* [PML_COMM_ID_BYTES] */);
int pml_comm_init(pml_ctx* ctx, int rank, int world, const unsigned char* id /* [PML_COMM_ID_BYTES] */);
int pml_comm_destroy(pml_ctx* ctx);
/*
 * What the attached communicator is, for a run's report (bench.py prints it in every N > 1 line so that the first run on a
 * real 8-GPU node can be read without a debugger): *rank, *world as given to pml_comm_init; *backend = 0 for a world of one
 * without librccl, 1 for RCCL; *rccl_ranks = what ncclCommCount says of the communicator (0 when backend == 0, -1 when the
 * loaded librccl has no ncclCommCount).  pml_device_uuid: the 16 bytes of hipDeviceGetUuid as 32 hex digits + NUL --
 * two ranks that report the same UUID share a GPU.
 */
int pml_comm_info(pml_ctx* ctx, int32_t* rank, int32_t* world, int32_t* backend, int32_t* rccl_ranks);
int pml_device_uuid(int device, char* uuid_out /* [33] */);
/* out[i] = sum / max over the ranks of in[i]; in and out are host arrays of count doubles (may alias); collective */
int pml_comm_allreduce(pml_ctx* ctx, const double* in, double* out, int32_t count, int op);
/*
 * total_out[0] = sum over all ranks of (loglik[0] + ... + loglik[n_cols-1]), loglik being this rank's pml_bottom_up
 * output: the forest-wide, all-character log-likelihood (the sum pastml/ml.py:112-121 forms per character, added up
 * over the characters of pastml/acr.py:226-231).  Collective.
 */
int pml_allreduce_loglik(pml_ctx* ctx, const double* loglik, int32_t n_cols, double* total_out);
/*
 * The same total without a host round trip of its own: when a communicator is attached, pml_marginal_pass forms the sum
 * of its columns' log-likelihoods on the device (column order), all-reduces it on the sweep's stream behind the sweeps
 * and copies it back before its one wait; pml_loglik_total hands that value out (once per pml_marginal_pass; every rank
 * must use the same route).
 */
int pml_loglik_total(pml_ctx* ctx, double* total_out);
/* hipDeviceSynchronize on the given device (benchmarks bracket their timed region with it) */
int pml_device_sync(int device);

/* ---- host-side helper of the optimiser loop (no GPU involved) -------------------------------------------------------- */
/*
 * The points of ONE forward-difference gradient of an F81-family character, decoded for the device, in one call: what
 * scipy's approx_derivative(method='2-point', abs_step=1e-8, bounds=...) evaluates around x -- x itself, then x + h_i e_i
 * with h_i = 1e-8 (the default L-BFGS-B differencing of pastml/ml.py:231) -- pushed through the model's parameter layout
 * (pastml/models/__init__.py:159-181, :328-330: x = [sf?] [tau?] [pi_0/pi_{k-1} .. pi_{k-2}/pi_{k-1}]?,
 * pi = (ratios, 1) / their sum with numpy's pairwise summation; tau factor of models/__init__.py:39-42).  Between two
 * sweeps of an optimiser round this arithmetic was a third of the host's time when done in numpy, a few small arrays at a
 * time.  n = len(x) = opt_sf + opt_tau + (free_pi ? k - 1 : 0); outputs: rows 0 .. n of pi_out[(n + 1) * k], sf_out,
 * tau_out, tf_out [n + 1] (row 0 = x itself) and steps_out[n] = (x_i + h_i) - x_i, the divisors of the differences.
 * Returns PML_OK, or PML_ERR_UNSUPPORTED when some x_i + h_i leaves [lower_i, upper_i] or equals x_i (scipy then mirrors
 * or rescales the step: the caller takes its general path) -- nothing is written in that case.
 * step: the absolute step h (1e-8 = scipy's; the polish run of a many-parameter search takes 1e-6).
 */
int pml_host_f81_fd_points(int32_t n, int32_t k, const double* x, const double* lower, const double* upper, int32_t opt_sf,
                           int32_t opt_tau, int32_t free_pi, double sf_fixed, double tau_fixed, const double* pi_fixed,
                           double forest_length, double num_nodes, double* pi_out, double* sf_out, double* tau_out,
                           double* tf_out, double* steps_out, double step);

/* ---- inspection ------------------------------------------------------------------------------------------------------ */
int pml_download(pml_ctx* ctx, int what, int32_t col, void* out);
/*
 * Rows first, first + stride, ... (count of them) of one column's buffer: what a caller that reports a sample of the
 * nodes needs (the marginal-probability table of named nodes, pastml/ml.py:486-502; validation of full-size runs)
 * without moving n_nodes * k doubles over PCIe.  what: PML_BUF_POSTERIOR (double[count][k]), PML_BUF_LH_SUM,
 * PML_BUF_LH_SF (double[count]) or PML_BUF_JOINT_STATE (int32[count]).
 */
int pml_download_strided(pml_ctx* ctx, int what, int32_t col, int32_t first, int32_t stride, int32_t count, void* out);
/* HIP-event timer on the ctx's stream */
int pml_timer_start(pml_ctx* ctx);
int pml_timer_stop(pml_ctx* ctx, float* milliseconds);
/*
 * Kernel-time accounting with HIP events on the ctx's stream (the stream the kernels are launched on).
 * While enabled, every pml_bottom_up / pml_top_down_marginals / pml_pij_batch call brackets its level-kernel
 * launches with an event pair and adds the elapsed time to an accumulator.
 * which: 0 = bottom-up level kernels, 1 = top-down level kernels, 2 = P(t) / prep kernels, 3 = the top-down launch of
 * the two-level units, 4 = their bottom-up launch (F81 family, level schedule of large forests; zero elsewhere).
 * launches counts kernel launches.  reset != 0 clears the accumulator after reading.
 */
int pml_profile_enable(pml_ctx* ctx, int on);
int pml_profile_read(pml_ctx* ctx, int which, double* total_ms, int64_t* launches, int reset);

#ifdef __cplusplus
}
#endif
#endif
