// libpastml_hip.so -- C-ABI (include/pastml_hip.h) over the HIP kernels: contexts, tree upload and schedules, the sweeps'
// launch sequences, downloads, the communicator.  The kernel families are launched through pml_launch.h; the entries that read
// what a marginal pass left on the device are pml_api_readers.hip's.  gfx950 only.
#define PML_PLAIN_KERNELS   // the kernels that are not templates are this unit's (pml_device.h, PML_GLOBAL)
#include "pml_launch.h"
#include "pml_kernels_eigen_gemm.h"   // (eig_sym_kernel)
#include "pml_comm.h"
#include "pml_pij_window.h"

// sha256 (first 16 hex digits) over the sources this library was compiled from, handed in by pastml_amd/build.py; the
// marker in front lets build.py read it out of the file without loading it
#ifndef PML_BUILD_DIGEST
#define PML_BUILD_DIGEST "unknown"
#endif
static const char kBuildDigest[] = "PML_BUILD_DIGEST=" PML_BUILD_DIGEST;

static thread_local std::string g_last_error;

int pml_fail(int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// rows of `width` elements between the caller's numbering and the library's, for n_cols columns of N rows each
template <typename T>
static void rows_to_internal(const pml_ctx* ctx, const T* api, T* internal, size_t width, size_t n_cols) {
    const size_t N = (size_t)ctx->N;
    for (size_t c = 0; c < n_cols; ++c)
        for (size_t q = 0; q < N; ++q)
            memcpy(internal + (c * N + q) * width, api + (c * N + (size_t)ctx->old_of_new[q]) * width, width * sizeof(T));
}

template <typename T>
static void rows_to_api(const pml_ctx* ctx, const T* internal, T* api, size_t width, size_t n_cols) {
    const size_t N = (size_t)ctx->N;
    for (size_t c = 0; c < n_cols; ++c)
        for (size_t q = 0; q < N; ++q)
            memcpy(api + (c * N + (size_t)ctx->old_of_new[q]) * width, internal + (c * N + q) * width, width * sizeof(T));
}

static inline bool permuted(const pml_ctx* ctx) { return !ctx->old_of_new.empty(); }

// an output that was fetched in the library's numbering, put into the caller's in place (after the copy has been waited for)
template <typename T>
static void rows_to_api_inplace(const pml_ctx* ctx, T* buf, size_t width, size_t n_cols) {
    if (!permuted(ctx) || buf == nullptr) return;
    const size_t col = (size_t)ctx->N * width;
    std::vector<T> tmp(col);   // (a column at a time: the table is never held twice)
    for (size_t c = 0; c < n_cols; ++c) {
        std::copy(buf + c * col, buf + (c + 1) * col, tmp.begin());
        rows_to_api(ctx, tmp.data(), buf + c * col, width, 1);
    }
}
// Per-node rows of n_cols columns from the device to the caller, in the caller's numbering: `width` elements of every row of
// `src_width` (the device pads rows to ks).  A renumbered forest's rows are gathered on the device, a column at a time, into a
// staging buffer of one column and copied from there -- no second copy of the table on the host, no serial host pass
// (round 5 permuted on the host after the copy: +8.6 GB of host memory for 32 columns of 262 144 tips at k = 64).
// Asynchronous on the ctx's stream; the caller synchronises.
template <typename T>
PML_INTERNAL int fetch_rows(pml_ctx* ctx, const T* d_src, size_t src_width, size_t width, size_t n_cols, T* out) {
    static_assert(sizeof(T) % 4 == 0, "rows are moved in 4-byte words");
    if (!out || n_cols == 0) return PML_OK;
    const size_t N = (size_t)ctx->N;
    if (!permuted(ctx)) {
        if (src_width == width)
            HIP_TRY(hipMemcpyAsync(out, d_src, n_cols * N * width * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(out, width * sizeof(T), d_src, src_width * sizeof(T), width * sizeof(T), n_cols * N,
                                     hipMemcpyDeviceToHost, ctx->stream));
        return PML_OK;
    }
    const size_t col_bytes = N * width * sizeof(T);
    if (ctx->stage_bytes < col_bytes) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (ctx->d_stage) (void)hipFree(ctx->d_stage);
        ctx->d_stage = nullptr;
        ctx->stage_bytes = 0;
        HIP_TRY(hipMalloc(&ctx->d_stage, col_bytes));
        ctx->stage_bytes = col_bytes;
    }
    const int wd = (int)(width * sizeof(T) / 4), ws = (int)(src_width * sizeof(T) / 4);
    const long long total = (long long)N * wd;
    const int blocks = (int)std::min<long long>((total + PML_BLOCK - 1) / PML_BLOCK, 65536);
    for (size_t c = 0; c < n_cols; ++c) {
        hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(PML_BLOCK), 0, ctx->stream,
                           (const unsigned*)(d_src + c * N * src_width), (unsigned*)ctx->d_stage, ctx->d_new_of_old, (long long)N, wd,
                           ws, 0, 1);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + c * N * width, ctx->d_stage, col_bytes, hipMemcpyDeviceToHost, ctx->stream));
    }
    return PML_OK;
}
template int fetch_rows<int>(pml_ctx*, const int*, size_t, size_t, size_t, int*);   // (pml_marginal_counts_altered's rows)

static inline int api_id(const pml_ctx* ctx, int internal) { return permuted(ctx) && internal >= 0 ? ctx->old_of_new[internal] : internal; }
static inline int internal_id(const pml_ctx* ctx, int api) { return permuted(ctx) && api >= 0 ? ctx->new_of_old[api] : api; }

// ---------------------------------------------------------------------------------------------------------------------
// The C-ABI: every pml_* function below is declared extern "C" in include/pastml_hip.h.

const char* pml_last_error(void) { return g_last_error.c_str(); }

int pml_version(void) { return PML_VERSION; }

const char* pml_build_digest(void) { return kBuildDigest + sizeof("PML_BUILD_DIGEST=") - 1; }

int pml_device_count(int* count) {
    if (!count) return fail(PML_ERR_INVALID, "count is NULL");
    HIP_TRY(hipGetDeviceCount(count));
    return PML_OK;
}

int pml_ctx_create(int device, pml_ctx** out) {
    if (!out) return fail(PML_ERR_INVALID, "out is NULL");
    *out = nullptr;
    // (the device list and the architecture names are asked for once per process: hipGetDeviceProperties costs ~10 ms,
    // and an analysis opens a context per group of characters)
    static std::mutex arch_lock;
    static std::vector<std::string> arch;
    {
        std::lock_guard<std::mutex> guard(arch_lock);
        if (arch.empty()) {
            int n = 0;
            HIP_TRY(hipGetDeviceCount(&n));
            std::vector<std::string> names;
            for (int d = 0; d < n; ++d) {
                hipDeviceProp_t prop;
                HIP_TRY(hipGetDeviceProperties(&prop, d));
                names.push_back(prop.gcnArchName);
            }
            arch.swap(names);
        }
    }
    const int n = (int)arch.size();
    if (device < 0 || device >= n) return fail(PML_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    HIP_TRY(hipSetDevice(device));
    if (strncmp(arch[device].c_str(), "gfx950", 6) != 0)
        return fail(PML_ERR_UNSUPPORTED, "device %d is %s; this library is built for gfx950 (MI355X) only", device,
                    arch[device].c_str());
    pml_ctx* ctx = new pml_ctx();
    ctx->device = device;
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev0);
    if (e == hipSuccess) e = hipEventCreate(&ctx->ev1);
    if (e != hipSuccess) {
        delete ctx;
        return fail(PML_ERR_HIP, "stream/event creation failed: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return PML_OK;
}

int pml_ctx_destroy(pml_ctx* ctx) {
    if (!ctx) return PML_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)pml_comm_destroy(ctx);
    free_all(ctx);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    prof_release(ctx);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PML_OK;
}

int pml_ctx_set_option(pml_ctx* ctx, int option, int value) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (option == PML_OPT_CHERRY_FUSION) {
        if (ctx->N != 0) return fail(PML_ERR_INVALID, "PML_OPT_CHERRY_FUSION must be set before the tree is uploaded");
        ctx->fuse = value != 0;
        return PML_OK;
    }
    if (option == PML_OPT_KEEP_TD) {
        if ((value != 0) != ctx->keep_td) {
            drop_graph(ctx->td_graph);
            drop_graph(ctx->mp_graph);
            ctx->results.tip_rows_unknown();   // (any change of an option: rare, and a blunt rule is enough)
        }
        ctx->keep_td = value != 0;
        return PML_OK;
    }
    if (option == PML_OPT_EIGEN_FUSED) {
        if ((value != 0) != ctx->eig_fused_opt) {
            drop_sweep_graphs(ctx);
            ctx->results.inputs_changed();
            ctx->results.tip_rows_unknown();
        }
        ctx->eig_fused_opt = value != 0;
        return PML_OK;
    }
    if (option == PML_OPT_EIGEN_JOINT_VALU) {
        if ((value != 0) != ctx->eigj_valu_opt) {
            drop_graph(ctx->bu_graph[0]);
            ctx->results.inputs_changed();
            ctx->results.tip_rows_unknown();
        }
        ctx->eigj_valu_opt = value != 0;
        return PML_OK;
    }
    if (option == PML_OPT_IMPLICIT_TIP_POSTERIORS) {
        if ((value != 0) != ctx->implicit_tips) {
            drop_graph(ctx->td_graph);
            drop_graph(ctx->mp_graph);
            ctx->results.tip_rows_unknown();   // (on: rows are left out of memory; off again: the next sweep writes them all)
        }
        ctx->implicit_tips = value != 0;
        return PML_OK;
    }
    return fail(PML_ERR_INVALID, "unknown option %d", option);
}

int pml_ctx_set_tunable(pml_ctx* ctx, const char* name, int64_t value, int is_set) {
    if (!ctx || !name) return fail(PML_ERR_INVALID, "ctx / name is NULL");
    if (strncmp(name, "PASTML_HIP_", 11) == 0) name += 11;
    for (int i = 0; i < T_COUNT; ++i) {
        if (strcmp(name, kTunableName[i]) != 0) continue;
        if (kTunableTree[i] && ctx->N != 0)
            return fail(PML_ERR_INVALID, "%s is read when the tree is uploaded: set it before pml_tree_upload", name);
        const bool on = is_set != 0 && (!kTunableFlag[i] || value != 0);
        ctx->tune.has[i] = on;
        ctx->tune.val[i] = on ? (long long)value : 0;
        // a captured launch sequence was made under the old setting
        drop_sweep_graphs(ctx);
        drop_graph(ctx->bt_graph);
        ctx->results.inputs_changed();
        ctx->results.tip_rows_unknown();
        return PML_OK;
    }
    return fail(PML_ERR_INVALID, "unknown tunable %s", name);
}

int pml_ctx_sync(pml_ctx* ctx) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PML_OK;
}

int pml_ctx_memory(pml_ctx* ctx, uint64_t* held, uint64_t* device_free) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    size_t f = 0, tot = 0;
    HIP_TRY(hipMemGetInfo(&f, &tot));
    if (held) *held = ctx->held;
    if (device_free) *device_free = f;
    return PML_OK;
}

static bool super_sweeps(const pml_ctx* ctx);

int pml_schedule_info(pml_ctx* ctx, int32_t* level_schedule, int32_t* n_two_level, int32_t* n_stacked) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    // (the model kind is set with the first model; until then the F81 family is assumed)
    const int kind = ctx->kind;
    if (kind < 0) ctx->kind = PML_MODEL_F81;
    const bool on = super_sweeps(ctx);
    ctx->kind = kind;
    if (level_schedule) *level_schedule = on ? 1 : 0;
    if (n_two_level) *n_two_level = on ? ctx->sup.n : 0;
    if (n_stacked) *n_stacked = on ? ctx->sup.n_stack : 0;
    return PML_OK;
}

int pml_tree_order(pml_ctx* ctx, int32_t* new_of_old) {
    if (!ctx || ctx->N == 0) return fail(PML_ERR_INVALID, "upload the tree first");
    if (!new_of_old) return fail(PML_ERR_INVALID, "new_of_old is NULL");
    for (int i = 0; i < ctx->N; ++i) new_of_old[i] = permuted(ctx) ? ctx->new_of_old[i] : i;
    return PML_OK;
}

int pml_sweep_schedule(pml_ctx* ctx, int32_t* kind, int32_t* n_blocks, int32_t* n_absorbed) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    const int model = ctx->kind;
    if (model < 0) ctx->kind = PML_MODEL_F81;  // (until the first model is set the F81 family is assumed)
    int k = PML_SCHEDULE_LEVELS;
    if (ctx->kind != PML_MODEL_F81) k = PML_SCHEDULE_OTHER_MODEL;
    else if (single_launch_sweeps(ctx)) k = PML_SCHEDULE_SINGLE_LAUNCH;
    else if (block_schedule(ctx)) k = PML_SCHEDULE_BLOCKS;
    else if (super_sweeps(ctx)) k = PML_SCHEDULE_TWO_LEVEL;
    ctx->kind = model;
    if (kind) *kind = k;
    if (n_blocks) *n_blocks = k == PML_SCHEDULE_BLOCKS ? ctx->blocks.n_blocks : 0;
    if (n_absorbed) *n_absorbed = 0;  // (the general two-level units of round 4 are gone: include/pastml_hip.h)
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// A tree: checked, numbered and planned on the host (pml_schedule.cpp), then the context is reset and every table of the
// tree is put on the device.
int pml_tree_upload(pml_ctx* ctx, int32_t n_nodes, int32_t n_roots, const int32_t* parent, const int32_t* first_child,
                    const int32_t* n_children, const double* dist, int32_t n_bu_levels, const int32_t* bu_offsets,
                    const int32_t* bu_order, int32_t n_td_levels, const int32_t* td_offsets,
                    const int32_t* td_parent_offsets, const int32_t* td_parents, const int32_t* post_rank) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    PmlTreeArrays t = {n_nodes,    n_roots,           n_bu_levels, n_td_levels, parent,    first_child, n_children,
                       bu_offsets, bu_order,          td_offsets,  td_parent_offsets, td_parents, post_rank, dist};
    const std::string bad = pml_check_tree(t);
    if (!bad.empty()) return fail(PML_ERR_INVALID, "%s", bad.c_str());
    // the library's own numbering (height_order): from here on every array is in it
    PmlNumbering num;
    PmlForest forest = pml_plan_forest(t, ctx->tune, ctx->fuse, num);
    PmlTreePlan P = pml_plan_tree(forest, t, ctx->tune);

    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    reset_for_tree(ctx);
    ctx->old_of_new.swap(num.old_of_new);
    ctx->new_of_old.swap(num.new_of_old);
    ctx->N = n_nodes;
    ctx->n_roots = n_roots;
    ctx->n_bu_levels = n_bu_levels;
    ctx->n_td_levels = n_td_levels;
    ctx->forest = std::move(forest);
    const PmlForest& f = ctx->forest;
    const int n_internal = f.n_internal, n_stored = f.n_stored();
    PML_TRY(put(ctx, &ctx->d_parent, t.parent, n_nodes));
    PML_TRY(put(ctx, &ctx->d_first_child, t.first_child, n_nodes));
    PML_TRY(put(ctx, &ctx->d_n_children, t.n_children, n_nodes));
    PML_TRY(put(ctx, &ctx->d_post_rank, t.post_rank, n_nodes));
    PML_TRY(put(ctx, &ctx->d_dist, t.dist, n_nodes));
    PML_TRY(put(ctx, &ctx->d_bu_order, t.bu_order, n_internal));
    PML_TRY(put(ctx, &ctx->d_td_parents, t.td_parents, n_internal));
    ctx->bu_order.assign(t.bu_order, t.bu_order + n_internal);   // (host copies: the window planner cuts these lists into runs)
    ctx->td_parents.assign(t.td_parents, t.td_parents + n_internal);
    if (permuted(ctx)) {
        PML_TRY(put(ctx, &ctx->d_new_of_old, ctx->new_of_old));
        PML_TRY(put(ctx, &ctx->d_old_of_new, ctx->old_of_new));
    }
    PML_TRY(put(ctx, &ctx->d_bu_offsets, f.bu_offsets));
    PML_TRY(put(ctx, &ctx->d_td_offsets, f.td_offsets));
    ctx->n_tips = (int)P.tips.size();
    PML_TRY(put(ctx, &ctx->d_tips, P.tips));
    // cherry fusion: kind per node, level lists over the stored internal nodes, unit descriptors of the lists
    ctx->n_cherries = (int)P.cherries.size();
    PML_TRY(put(ctx, &ctx->d_kind, f.kind));
    PML_TRY(put(ctx, &ctx->d_bu_order_f, f.order_f));
    PML_TRY(put(ctx, &ctx->d_td_parents_f, f.tdp));
    PML_TRY(put(ctx, &ctx->d_cherries, P.cherries));
    PML_TRY(put(ctx, &ctx->d_bu_offsets_f, f.bu_offsets_f));
    PML_TRY(put(ctx, &ctx->d_td_parent_offsets_f, f.td_parent_offsets_f));
    PML_TRY(put(ctx, &ctx->d_cherry_units, P.cherry_units));
    PML_TRY(put(ctx, &ctx->d_bu_units_f, P.bu_units_f));
    PML_TRY(put(ctx, &ctx->d_td_units_f, P.td_units_f));
    PML_TRY(put(ctx, &ctx->d_bu_units, P.bu_units));
    if (P.shape_sort) {
        PML_TRY(put(ctx, &ctx->d_bu_units_fs, P.bu_units_fs));
        PML_TRY(put(ctx, &ctx->d_td_units_fs, P.td_units_fs));
    }
    ctx->bu_level_vec_f.swap(P.bu_level_vec_f);
    ctx->bu_level_vec.swap(P.bu_level_vec);
    ctx->td_cherry_prefix.swap(P.td_cherry_prefix);
    ctx->small = P.small;
    // the schedules: their geometry as planned, their tables on the device
    pml_ctx::EigenTiers& E = ctx->eig_tiers;
    E = P.eig.s;
    if (E.ok) {
        PML_TRY(put(ctx, &E.d_nodes, P.eig.t.list));
        PML_TRY(put(ctx, &E.d_units, P.eig.units));
        PML_TRY(put(ctx, &E.d_lv, P.eig.t.lv));
        PML_TRY(put(ctx, &E.d_start, P.eig.t.start));
    }
    pml_ctx::BacktraceTiers& T = ctx->bt_tiers;
    T = P.bt.s;
    if (T.ok) {
        PML_TRY(put(ctx, &T.d_nodes, P.bt.t.list));
        PML_TRY(put(ctx, &T.d_lv, P.bt.t.lv));
        PML_TRY(put(ctx, &T.d_start, P.bt.t.start));
    }
    pml_ctx::SuperSchedule& U = ctx->sup;
    U = P.sup.s;
    if (U.n_stack > 0) {
        PML_TRY(put(ctx, &U.d_stack_bu, P.sup.stack_bu));
        PML_TRY(put(ctx, &U.d_stack_td, P.sup.stack_td));
        PML_TRY(put(ctx, &U.d_stack_children, P.sup.stack_children));
    }
    if (P.sup.lists) {
        PML_TRY(put(ctx, &U.d_child_units, P.sup.child_units));
        PML_TRY(put(ctx, &U.d_units, P.sup.units));
        PML_TRY(put(ctx, &U.d_bu_units_r, P.sup.bu_units_r));
        PML_TRY(put(ctx, &U.d_td_units_r, P.sup.td_units_r));
        if (P.shape_sort) {
            PML_TRY(put(ctx, &U.d_bu_units_rs, P.sup.bu_units_rs));
            PML_TRY(put(ctx, &U.d_td_units_rs, P.sup.td_units_rs));
        }
        PML_TRY(put(ctx, &U.d_bu_offsets_r, U.bu_offsets_r));
        PML_TRY(put(ctx, &U.d_td_offsets_r, U.td_offsets_r));
    }
    pml_ctx::BlockSchedule& B = ctx->blocks;
    B = P.blocks.s;
    if (B.ok) {
        PML_TRY(put(ctx, &B.d_bu_units, P.blocks.bu_units));
        PML_TRY(put(ctx, &B.d_td_units, P.blocks.td_units));
        PML_TRY(put(ctx, &B.d_top_bu_units, P.blocks.top_bu_units));
        PML_TRY(put(ctx, &B.d_top_td_units, P.blocks.top_td_units));
        PML_TRY(put(ctx, &B.d_bu_start, P.blocks.bu.start));
        PML_TRY(put(ctx, &B.d_bu_levels, P.blocks.bu.levels));
        PML_TRY(put(ctx, &B.d_bu_lv, P.blocks.bu.lv));
        PML_TRY(put(ctx, &B.d_td_start, P.blocks.td.start));
        PML_TRY(put(ctx, &B.d_td_levels, P.blocks.td.levels));
        PML_TRY(put(ctx, &B.d_td_lv, P.blocks.td.lv));
        PML_TRY(put(ctx, &B.d_top_bu_offsets, B.top_bu_offsets));
        PML_TRY(put(ctx, &B.d_top_td_offsets, B.top_td_offsets));
    }
    // the unit lists and their level tables by PmlList; a list sorted by shape is the plain one where the forest has none
    auto or_else = [](const PmlUnit* sorted, const PmlUnit* plain) { return sorted ? sorted : plain; };
    const PmlUnit** L = ctx->d_unit_lists;
    L[L_BU_FUSED] = ctx->d_bu_units_f;
    L[L_BU_FUSED_SORTED] = or_else(ctx->d_bu_units_fs, ctx->d_bu_units_f);
    L[L_TD_FUSED] = ctx->d_td_units_f;
    L[L_TD_FUSED_SORTED] = or_else(ctx->d_td_units_fs, ctx->d_td_units_f);
    L[L_BU_PLAIN] = ctx->d_bu_units;
    L[L_CHERRIES] = ctx->d_cherry_units;
    L[L_TOP_BU] = B.d_top_bu_units;
    L[L_TOP_TD] = B.d_top_td_units;
    L[L_REST_BU] = U.d_bu_units_r;
    L[L_REST_BU_SORTED] = or_else(U.d_bu_units_rs, U.d_bu_units_r);
    L[L_REST_TD] = U.d_td_units_r;
    L[L_REST_TD_SORTED] = or_else(U.d_td_units_rs, U.d_td_units_r);
    L[L_CHILD_UNITS] = U.d_child_units;
    L[L_STACK_CHILDREN] = U.d_stack_children;
    ctx->d_list_offsets[L_BU_FUSED] = ctx->d_bu_offsets_f;
    ctx->d_list_offsets[L_TD_FUSED] = ctx->d_td_parent_offsets_f;
    ctx->d_list_offsets[L_TOP_BU] = B.d_top_bu_offsets;
    ctx->d_list_offsets[L_TOP_TD] = B.d_top_td_offsets;
    ctx->d_list_offsets[L_REST_BU] = U.d_bu_offsets_r;
    ctx->d_list_offsets[L_REST_TD] = U.d_td_offsets_r;
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host tables go out of scope)
    return PML_OK;
}

// The thin ends of a large forest (pml_plan_thin_ends); thin: the most units a thin level holds (pml_plan_columns: by the
// bytes a level of that many units moves).
static int build_thin_ends(pml_ctx* ctx, int thin) {
    PmlThinPlan P = pml_plan_thin_ends(ctx->forest, ctx->tune, thin);
    pml_ctx::ThinSchedule& H = ctx->thin;
    pml_ctx::DeepSchedule& D = ctx->deep;
    H = P.thin;
    D = P.deep;
    if (H.ok) {
        PML_TRY(put(ctx, &H.d_units, P.bu_units));
        PML_TRY(put(ctx, &H.d_start, P.bu.start));
        PML_TRY(put(ctx, &H.d_levels, P.bu.levels));
        PML_TRY(put(ctx, &H.d_lv, P.bu.lv));
    }
    if (D.ok) {
        PML_TRY(put(ctx, &D.d_units, P.td_units));
        PML_TRY(put(ctx, &D.d_start, P.td.start));
        PML_TRY(put(ctx, &D.d_levels, P.td.levels));
        PML_TRY(put(ctx, &D.d_lv, P.td.lv));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // (the host tables go out of scope)
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
static_assert(PML_COLUMNS_MAX_STATES == PML_MAX_STATES, "the column planner and the kernels disagree on the most states");
// pml_plan_columns' reasons: a bad argument is invalid, a layout the kernels cannot hold or address unsupported
static int column_plan_status(const std::string& why) {
    return why.rfind("k = ", 0) == 0 || why.rfind("n_nodes", 0) == 0 ? PML_ERR_UNSUPPORTED : PML_ERR_INVALID;
}

// Plans the layout (pml_plan_columns: every rule is there), then allocates and fills what the plan describes.
int pml_chars_alloc(pml_ctx* ctx, int32_t n_cols, int32_t k) {
    if (!ctx || ctx->N == 0) return fail(PML_ERR_INVALID, "upload the tree first");
    if (ctx->C != 0) return fail(PML_ERR_INVALID, "columns already allocated for this tree (upload the tree again to reset)");
    PmlColumnPlan plan;
    const std::string why = pml_plan_columns(ctx->forest, ctx->tune, n_cols, k, plan);
    if (!why.empty()) return fail(column_plan_status(why), "%s", why.c_str());
    HIP_TRY(hipSetDevice(ctx->device));
    ctx->cols = plan;
    ctx->C = plan.C;
    ctx->k = plan.k;
    ctx->ks = plan.ks;
    ctx->W = plan.W;
    const PmlParamBlock& B = plan.params;
    const size_t CN = (size_t)n_cols * ctx->N;
    PML_TRY(dev_alloc(ctx, &ctx->d_masks, CN * ctx->W));
    PML_TRY(dev_alloc(ctx, &ctx->d_params, B.count));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_params, sizeof(double) * B.count));
    memset(ctx->h_params, 0, sizeof(double) * B.count);
    std::fill_n(ctx->h_params + B.active, n_cols, 1.0);  // every column active
    ctx->d_pi = ctx->d_params + B.pi;
    ctx->d_sf = ctx->d_params + B.sf;
    ctx->d_tau = ctx->d_params + B.tau;
    ctx->d_tauf = ctx->d_params + B.tauf;
    ctx->d_mu = ctx->d_params + B.mu;
    ctx->d_kappa = ctx->d_params + B.kappa;
    ctx->d_active = ctx->d_params + B.active;
    ctx->active_partial = false;
    ctx->n_active = ctx->sched_cols = n_cols;
    PML_TRY(dev_alloc(ctx, &ctx->d_err, n_cols));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_loglik, sizeof(double) * n_cols + sizeof(u64)));
    ctx->h_bad_tip = reinterpret_cast<u64*>(ctx->h_loglik + n_cols);
    *ctx->h_bad_tip = 0;
    HIP_TRY(hipHostMalloc((void**)&ctx->h_err, sizeof(u64) * n_cols));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_done, 64));
    *ctx->h_done = 0;
    PML_TRY(dev_alloc(ctx, &ctx->d_done, 2));
    HIP_TRY(hipMemsetAsync(ctx->d_done, 0, 2 * sizeof(u64), ctx->stream));
    ctx->pending = {};
    ctx->graphs = !ctx->tune.on(T_NO_GRAPH);
    PML_TRY(dev_alloc(ctx, &ctx->d_bu, CN * ctx->ks));
    PML_TRY(dev_alloc(ctx, &ctx->d_S, CN));
    PML_TRY(dev_alloc(ctx, &ctx->d_be, CN));
    PML_TRY(dev_alloc(ctx, &ctx->d_E, CN));
    HIP_TRY(hipMemcpyAsync(ctx->d_params, ctx->h_params, ctx->cols.params.count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(ctx->d_be, 0, CN * sizeof(i64), ctx->stream));
    // default masks: everything allowed
    {
        dim3 grid(grid_for(ctx, (int)std::min<size_t>((size_t)ctx->N * ctx->W, 1u << 30), PML_BLOCK, n_cols), n_cols);
        hipLaunchKernelGGL(masks_fill_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, ctx->N, ctx->W, ctx->k,
                           ctx->d_masks, 0);
        HIP_TRY(hipGetLastError());
    }
    ctx->model_set.assign(n_cols, 0);
    ctx->eig_sym.assign(n_cols, 0);
    ctx->eig_sym_all = false;
    ctx->tips_observed.assign(n_cols, 0);
    ctx->results.inputs_changed();
    ctx->results.tip_rows_unknown();   // (the table is allocated anew)
    if (plan.thin_units > 0) PML_TRY(build_thin_ends(ctx, plan.thin_units));
    return PML_OK;
}

PML_INTERNAL int check_cols(pml_ctx* ctx, int cb, int ce) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    if (cb < 0 || ce > ctx->C || cb >= ce) return fail(PML_ERR_INVALID, "column range [%d, %d) out of 0..%d", cb, ce, ctx->C);
    HIP_TRY(hipSetDevice(ctx->device));
    return PML_OK;
}

// PML_OPT_IMPLICIT_TIP_POSTERIORS: whoever reads the posterior table gets the rows the sweep left implicit first
PML_INTERNAL int materialize_tip_posteriors(pml_ctx* ctx) {
    if (!ctx->results.tip_posteriors_missing() || !ctx->d_post || ctx->n_tips == 0) return PML_OK;
    dim3 grid(grid_for(ctx, ctx->n_tips, PML_BLOCK, ctx->C), ctx->C);
    hipLaunchKernelGGL(tip_posteriors_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, cols_of(ctx), state_of(ctx), ctx->N,
                       ctx->d_tips, ctx->n_tips);
    HIP_TRY(hipGetLastError());
    ctx->results.tip_posteriors_written();
    return PML_OK;
}

// what is known about the tips of columns [col_begin, col_end); the captured launch sequence of the joint sweep depends
// on whether ALL columns' tips are observed (launch_eigen_joint_tips), so a change of that drops the graph
static void note_tips_observed(pml_ctx* ctx, int col_begin, int col_end, bool observed) {
    auto all = [&]() {
        bool a = !ctx->tips_observed.empty();
        for (char f : ctx->tips_observed) a = a && f != 0;
        return a;
    };
    const bool before = all();
    for (int col = col_begin; col < col_end; ++col) ctx->tips_observed[col] = observed ? 1 : 0;
    if (all() != before) drop_graph(ctx->bu_graph[0]);
}

int pml_masks_upload(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint64_t* masks) {
    PML_TRY(check_cols(ctx, col_begin, col_end));
    PML_TRY(materialize_tip_posteriors(ctx));  // (rows left implicit are defined by the masks about to change)
    if (!masks) return fail(PML_ERR_INVALID, "masks is NULL");
    const size_t per_col = (size_t)ctx->N * ctx->W;
    // bits beyond k must be clear: the kernels trust the words
    if (ctx->k % 64) {
        const u64 valid = (1ull << (ctx->k % 64)) - 1ull;
        const size_t n = per_col * (col_end - col_begin);
        for (size_t i = ctx->W - 1; i < n; i += ctx->W)
            if (masks[i] & ~valid) return fail(PML_ERR_INVALID, "mask word %zu has bits beyond k = %d", i, ctx->k);
    }
    std::vector<u64> reordered;   // (the caller's rows in the library's numbering; alive until the copy below has been waited for)
    const u64* src = (const u64*)masks;
    if (permuted(ctx)) {
        reordered.resize(per_col * (col_end - col_begin));
        rows_to_internal(ctx, src, reordered.data(), (size_t)ctx->W, (size_t)(col_end - col_begin));
        src = reordered.data();
    }
    ctx->results.tip_rows_unknown();   // (before the write: whichever columns and nodes it changes, and whether it goes through)
    PML_TRY(upload(ctx, ctx->d_masks + col_begin * per_col, src, per_col * (col_end - col_begin)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    note_tips_observed(ctx, col_begin, col_end, false);
    ctx->results.inputs_changed();
    return PML_OK;
}

int pml_masks_from_tip_states(pml_ctx* ctx, int32_t col_begin, int32_t col_end, int32_t n_tips,
                              const int32_t* tip_ids, const int32_t* states) {
    PML_TRY(check_cols(ctx, col_begin, col_end));
    PML_TRY(materialize_tip_posteriors(ctx));
    if (n_tips < 0 || (n_tips > 0 && (!tip_ids || !states))) return fail(PML_ERR_INVALID, "bad tip arrays");
    const int nc = col_end - col_begin;
    std::vector<int32_t> own_ids;   // the caller's tip ids in the library's numbering
    for (int j = 0; j < n_tips; ++j)
        if (tip_ids[j] < 0 || tip_ids[j] >= ctx->N || ctx->forest.n_children[internal_id(ctx, tip_ids[j])] != 0)
            return fail(PML_ERR_INVALID, "tip_ids[%d] = %d is not a tip", j, tip_ids[j]);
    if (permuted(ctx) && n_tips > 0) {
        own_ids.resize(n_tips);
        for (int j = 0; j < n_tips; ++j) own_ids[j] = ctx->new_of_old[tip_ids[j]];
        tip_ids = own_ids.data();
    }
    for (size_t i = 0; i < (size_t)nc * n_tips; ++i)
        if (states[i] >= ctx->k) return fail(PML_ERR_INVALID, "state %d out of range (k = %d)", states[i], ctx->k);
    ctx->results.tip_rows_unknown();   // (before the write, as pml_masks_upload)
    dim3 grid(grid_for(ctx, (int)std::min<size_t>((size_t)ctx->N * ctx->W, 1u << 30), PML_BLOCK, nc), nc);
    hipLaunchKernelGGL(masks_fill_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, ctx->N, ctx->W, ctx->k, ctx->d_masks,
                       col_begin);
    HIP_TRY(hipGetLastError());
    if (n_tips > 0) {
        CallScope mem(ctx->stream, false);   // (tip_ids may be own_ids, declared above)
        int *d_ids, *d_states;
        PML_TRY(mem.put(&d_ids, tip_ids, (size_t)n_tips));
        PML_TRY(mem.put(&d_states, states, (size_t)nc * n_tips));
        dim3 g2(grid_for(ctx, n_tips, PML_BLOCK, nc), nc);
        hipLaunchKernelGGL(masks_tips_kernel, g2, dim3(PML_BLOCK), 0, ctx->stream, ctx->N, ctx->W, ctx->k,
                           ctx->d_masks, col_begin, n_tips, d_ids, d_states);
        HIP_TRY(hipGetLastError());
        PML_TRY(mem.finish());
    }
    for (int col = col_begin; col < col_end; ++col) {
        bool all = n_tips == ctx->n_tips;   // (the ids are distinct tips or the masks would not be what the caller meant)
        for (int j = 0; all && j < n_tips; ++j) all = states[(size_t)(col - col_begin) * n_tips + j] >= 0;
        note_tips_observed(ctx, col, col + 1, all);
    }
    ctx->results.inputs_changed();
    return PML_OK;
}

int pml_masks_initial_upload(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const uint64_t* masks) {
    PML_TRY(check_cols(ctx, col_begin, col_end));
    if (!masks) {
        ctx->has_init = false;
        return PML_OK;
    }
    const size_t per_col = (size_t)ctx->N * ctx->W;
    if (!ctx->d_masks_init) {
        PML_TRY(dev_alloc(ctx, &ctx->d_masks_init, per_col * ctx->C));
        // columns never given initial masks compare equal to nothing altered: start from the current masks
        HIP_TRY(hipMemcpyAsync(ctx->d_masks_init, ctx->d_masks, per_col * ctx->C * sizeof(u64), hipMemcpyDeviceToDevice,
                               ctx->stream));
    }
    if (ctx->k % 64) {
        const u64 valid = (1ull << (ctx->k % 64)) - 1ull;
        const size_t n = per_col * (col_end - col_begin);
        for (size_t i = ctx->W - 1; i < n; i += ctx->W)
            if (masks[i] & ~valid) return fail(PML_ERR_INVALID, "mask word %zu has bits beyond k = %d", i, ctx->k);
    }
    std::vector<u64> reordered;
    const u64* src = (const u64*)masks;
    if (permuted(ctx)) {
        reordered.resize(per_col * (col_end - col_begin));
        rows_to_internal(ctx, src, reordered.data(), (size_t)ctx->W, (size_t)(col_end - col_begin));
        src = reordered.data();
    }
    PML_TRY(upload(ctx, ctx->d_masks_init + col_begin * per_col, src, per_col * (col_end - col_begin)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->has_init = true;
    ctx->results.initial_masks_changed();
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
static int set_common(pml_ctx* ctx, int kind, int cb, int ce, const double* pi, const double* sf, const double* tau,
                      const double* tauf) {
    PML_TRY(check_cols(ctx, cb, ce));
    if (!pi || !sf || !tau || !tauf) return fail(PML_ERR_INVALID, "NULL parameter array");
    if (ctx->kind != -1 && ctx->kind != kind) {
        // one model kind per ctx; setting ALL columns at once may change it (a pooled ctx serving the next analysis)
        if (cb != 0 || ce != ctx->C) return fail(PML_ERR_INVALID, "all columns of a ctx must use one model kind");
        drop_sweep_graphs(ctx);
        ctx->results.tip_rows_unknown();
    }
    if (kind == PML_MODEL_HKY && ctx->k != 4) return fail(PML_ERR_INVALID, "HKY needs k = 4");
    const int nc = ce - cb;
    for (int i = 0; i < nc; ++i)
        if (!(sf[i] > 0.0) || !(tau[i] >= 0.0) || !(tauf[i] > 0.0) || !std::isfinite(sf[i]) || !std::isfinite(tau[i]))
            return fail(PML_ERR_INVALID, "bad sf/tau/tau_factor for column %d", cb + i);
    ctx->kind = kind;
    // into the pinned mirror (the caller's arrays need not outlive the call); params_flush sends it
    double* h = ctx->h_params;
    const size_t ks = ctx->ks, k = ctx->k;
    for (int i = 0; i < nc; ++i) {
        double* row = h + (size_t)(cb + i) * ks;
        memcpy(row, pi + (size_t)i * k, k * sizeof(double));
        for (size_t q = k; q < ks; ++q) row[q] = 0.0;
    }
    const PmlParamBlock& B = ctx->cols.params;
    memcpy(h + B.sf + cb, sf, nc * sizeof(double));
    memcpy(h + B.tau + cb, tau, nc * sizeof(double));
    memcpy(h + B.tauf + cb, tauf, nc * sizeof(double));
    for (int i = cb; i < ce; ++i) ctx->model_set[i] = 1;
    ctx->results.inputs_changed();
    return PML_OK;
}

// One asynchronous copy of the parameter block (small: (k + 5) doubles per column).  A copy still in flight when the
// mirror is written again is harmless: copies are stream-ordered and the later one carries the final contents.
// A parameter update only marks the pinned mirror; the copy goes out with the next sweep (params_push) -- inside its
// graph when the sweep is replayed as one, so that an optimiser step is ONE call into the runtime (a graph launch) instead
// of two (≈4 us of a 90 us pass on the latency-bound configurations).  The mirror is not touched while a sweep is in
// flight: every sweep is waited for before its results are used, and parameters change between sweeps.
static int params_flush(pml_ctx* ctx) {
    ctx->params_dirty = true;
    return PML_OK;
}

// (captured: the copy is recorded whatever the mirror holds now, and the sequence's outcome says that it is part of it --
// the mirror counts as sent whenever the graph is launched, run_captured)
static int params_push(pml_ctx* ctx, PmlCapture capture = CAP_NONE, PmlSweepOutcome* outcome = nullptr) {
    if (capture == CAP_NONE && !ctx->params_dirty) return PML_OK;
    HIP_TRY(hipMemcpyAsync(ctx->d_params, ctx->h_params, ctx->cols.params.count * sizeof(double), hipMemcpyHostToDevice,
                           ctx->stream));
    if (capture == CAP_NONE) ctx->params_dirty = false;
    else if (outcome) outcome->has_params = true;
    return PML_OK;
}

int pml_model_set_f81(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi, const double* sf,
                      const double* tau, const double* tau_factor) {
    PML_TRY(set_common(ctx, PML_MODEL_F81, col_begin, col_end, pi, sf, tau, tau_factor));
    const int nc = col_end - col_begin;
    double* mu = ctx->h_params + ctx->cols.params.mu + col_begin;
    for (int c = 0; c < nc; ++c) {
        // mu = 1 / (1 - sum pi^2), F81Model.py:18-26 (numpy dot)
        double dot = 0.0;
        for (int s = 0; s < ctx->k; ++s) dot += pi[(size_t)c * ctx->k + s] * pi[(size_t)c * ctx->k + s];
        mu[c] = 1.0 / (1.0 - dot);
    }
    return params_flush(ctx);
}

int pml_model_set_hky(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi, const double* kappa,
                      const double* sf, const double* tau, const double* tau_factor) {
    if (!kappa) return fail(PML_ERR_INVALID, "kappa is NULL");
    PML_TRY(set_common(ctx, PML_MODEL_HKY, col_begin, col_end, pi, sf, tau, tau_factor));
    memcpy(ctx->h_params + ctx->cols.params.kappa + col_begin, kappa, (col_end - col_begin) * sizeof(double));
    return params_flush(ctx);
}

int pml_model_set_eigen(pml_ctx* ctx, int32_t col_begin, int32_t col_end, const double* pi, const double* d,
                        const double* A, const double* Ainv, const double* sf, const double* tau,
                        const double* tau_factor) {
    if (!d || !A || !Ainv) return fail(PML_ERR_INVALID, "NULL eigen array");
    if (ctx && ctx->k > PML_MAX_STATES_MATRIX)
        return fail(PML_ERR_UNSUPPORTED, "k = %d states: the eigen-decomposed models take at most %d (the F81 family %d)", ctx->k,
                    PML_MAX_STATES_MATRIX, PML_MAX_STATES);
    PML_TRY(set_common(ctx, PML_MODEL_EIGEN, col_begin, col_end, pi, sf, tau, tau_factor));
    const size_t k = ctx->k;
    if (!ctx->d_d) {
        PML_TRY(dev_alloc(ctx, &ctx->d_d, (size_t)ctx->C * k));
        PML_TRY(dev_alloc(ctx, &ctx->d_A, (size_t)ctx->C * k * k));
        PML_TRY(dev_alloc(ctx, &ctx->d_Ainv, (size_t)ctx->C * k * k));
    }
    const int nc = col_end - col_begin;
    PML_TRY(params_flush(ctx));
    PML_TRY(upload(ctx, ctx->d_d + col_begin * k, d, nc * k));
    if (ctx->h_eig_d.size() != (size_t)ctx->C * k) ctx->h_eig_d.assign((size_t)ctx->C * k, 0.0);
    memcpy(ctx->h_eig_d.data() + col_begin * k, d, nc * k * sizeof(double));
    PML_TRY(upload(ctx, ctx->d_A + col_begin * k * k, A, nc * k * k));
    PML_TRY(upload(ctx, ctx->d_Ainv + col_begin * k * k, Ainv, nc * k * k));
    if (k > 64 && k <= 128) {
        // More than 64 states: the sum sweeps keep ONE matrix in LDS (pml_kernels_eigen_gemm.h, EigGemm::SYM), which needs
        //   Ainv[m][j] = c_m A[j][m] pi[j],  c_m = 1 / sum_j pi[j] A[j][m]^2
        // -- true of a reversible model's eigenvectors (generator.py:33-51 builds nothing else) unless an eigenvalue repeats and
        // numpy left its eigenvectors far from orthogonal.  Checked entry by entry on what was handed in (to 1e-8: what is left
        // below that is numpy's rounding, which eig_sym_kernel's Newton-Schulz step removes); the sweeps of a ctx with a column
        // that fails read materialised P(t).
        if (!ctx->d_Asym) {
            PML_TRY(dev_alloc(ctx, &ctx->d_Asym, (size_t)ctx->C * k * k));
            PML_TRY(dev_alloc(ctx, &ctx->d_eigT, (size_t)ctx->C * k * k));
        }
        for (int c = 0; c < nc; ++c) {
            const double *Ac = A + (size_t)c * k * k, *Bc = Ainv + (size_t)c * k * k, *pc = pi + (size_t)c * k;
            bool ok = true;
            for (size_t j = 0; j < k; ++j) ok = ok && pc[j] > 0.0;
            for (size_t mm = 0; mm < k && ok; ++mm) {
                double g = 0.0, big = 0.0;
                for (size_t j = 0; j < k; ++j) {
                    g += pc[j] * Ac[j * k + mm] * Ac[j * k + mm];
                    big = std::max(big, std::fabs(Bc[mm * k + j]));
                }
                const double cm = 1.0 / g;
                if (!(g > 0.0) || !std::isfinite(cm)) ok = false;
                for (size_t j = 0; j < k && ok; ++j)
                    if (!(std::fabs(Bc[mm * k + j] - cm * Ac[j * k + mm] * pc[j]) <= 1e-8 * big)) ok = false;
            }
            ctx->eig_sym[col_begin + c] = ok ? 1 : 0;
        }
        // (an optimiser that moves the scaling factor alone hands in the same matrices evaluation after evaluation)
        const size_t kk = k * k;
        if (ctx->h_symA.size() != (size_t)ctx->C * (kk + k)) ctx->h_symA.assign((size_t)ctx->C * (kk + k), 0.0);
        bool same = true;
        for (int c = 0; c < nc; ++c) {
            double* last = ctx->h_symA.data() + (size_t)(col_begin + c) * (kk + k);
            if (memcmp(last, A + (size_t)c * kk, kk * sizeof(double)) != 0 || memcmp(last + kk, pi + (size_t)c * k, k * sizeof(double)) != 0) {
                same = false;
                memcpy(last, A + (size_t)c * kk, kk * sizeof(double));
                memcpy(last + kk, pi + (size_t)c * k, k * sizeof(double));
            }
        }
        if (!same) {
            PML_TRY(params_push(ctx));   // (the kernel reads the frequencies from the parameter block)
            const size_t lds = (k * (k + 1) + k) * sizeof(double);
            PML_TRY(with_lds(ctx, eig_sym_kernel, lds));
            for (int phase = 0; phase < 2; ++phase)
                hipLaunchKernelGGL(eig_sym_kernel, dim3(PML_ESYM_PARTS, nc), dim3(PML_BLOCK), lds, ctx->stream, (int)k, ctx->ks,
                                   (int)col_begin, phase, ctx->d_A, cols_of(ctx).pi, ctx->d_eigT, ctx->d_Asym);
            HIP_TRY(hipGetLastError());
        }
        bool all = true;
        for (int i = 0; i < ctx->C; ++i) all = all && (ctx->eig_sym[i] != 0 || !ctx->model_set[i]);
        if (all != ctx->eig_sym_all) drop_sweep_graphs(ctx);   // the sweeps change kernels
        ctx->eig_sym_all = all;
    }
    std::vector<double> at, a_t;
    if (k <= 64) {
        // transposed, zero-padded copies: A^-1 for the joint sweep on the vector units (k <= 32: its rows through the scalar cache) and
        // for the observed tips of the sum sweeps (a column of A^-1 is a contiguous row here); A for the P(t) batch below 16 states
        const size_t ld = k <= PML_EIGJ_STRIDE ? PML_EIGJ_STRIDE : 64, sq = ld * ld;
        if (!ctx->d_AinvT) PML_TRY(dev_alloc(ctx, &ctx->d_AinvT, (size_t)ctx->C * sq));
        at.assign((size_t)nc * sq, 0.0);
        for (int c = 0; c < nc; ++c)
            for (size_t mm = 0; mm < k; ++mm)
                for (size_t j = 0; j < k; ++j)
                    at[c * sq + j * ld + mm] = Ainv[(size_t)c * k * k + mm * k + j];
        PML_TRY(upload(ctx, ctx->d_AinvT + (size_t)col_begin * sq, at.data(), at.size()));
        if (k <= PML_EIGJ_STRIDE) {
            if (!ctx->d_AT) PML_TRY(dev_alloc(ctx, &ctx->d_AT, (size_t)ctx->C * sq));
            a_t.assign((size_t)nc * sq, 0.0);
            for (int c = 0; c < nc; ++c)
                for (size_t i = 0; i < k; ++i)
                    for (size_t mm = 0; mm < k; ++mm)
                        a_t[c * sq + mm * ld + i] = A[(size_t)c * k * k + i * k + mm];
            PML_TRY(upload(ctx, ctx->d_AT + (size_t)col_begin * sq, a_t.data(), a_t.size()));
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
PML_INTERNAL int require_model(pml_ctx* ctx) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    for (int i = 0; i < ctx->C; ++i)
        if (!ctx->model_set[i]) return fail(PML_ERR_INVALID, "model parameters of column %d were never set", i);
    HIP_TRY(hipSetDevice(ctx->device));
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// P(t) in a window (pml_pij_window.h).  The plans the branch lists are cut from are those of the sweeps that read P(t): the
// plain level launches, whatever the switches of the fused sweeps say -- a sweep's own plan, cut again when it is enqueued
// (run_plan), must list the same branches.
static PmlSweepTraits sweep_traits(const pml_ctx* ctx);
static PmlSchedules schedules_of(const pml_ctx* ctx);

static void window_drop(pml_ctx* ctx) {
    const size_t kk = (size_t)ctx->k * ctx->ks;
    dev_release(ctx, &ctx->d_pij_window, (size_t)ctx->C * (size_t)ctx->pij_window * kk);
    for (int i = 0; i < 2; ++i) {
        dev_release(ctx, &ctx->d_win_branches[i], ctx->win_branches[i].size());
        dev_release(ctx, &ctx->d_win_slot[i], (size_t)ctx->N);
        ctx->win_branches[i].clear();
    }
    ctx->win_cuts.clear();
    ctx->win_td_runs.clear();
    ctx->pij_window = 0;
}

static int window_set(pml_ctx* ctx, long long branches) {
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->pending.spin = false;
    // a captured launch sequence was made for the other source of P(t)
    drop_sweep_graphs(ctx);
    ctx->results.pij_source_changed();
    window_drop(ctx);
    if (branches == 0) return PML_OK;
    const long long B = std::min<long long>(branches, ctx->N);
    PmlSweepTraits t = sweep_traits(ctx);
    t.eigen_fused = t.eigen_gemm = t.eigen_joint_valu = t.hky_fused = false;
    PmlWindowPlan W[2];
    const std::vector<PmlLaunch> plans[2] = {pml_plan_bottom_up(ctx->forest, schedules_of(ctx), t, false),
                                             pml_plan_top_down(ctx->forest, schedules_of(ctx), t, false)};
    for (int i = 0; i < 2; ++i) {
        const std::string bad = pml_plan_pij_window(plans[i], ctx->forest, ctx->bu_order, ctx->td_parents, B, W[i]);
        if (!bad.empty()) return fail(PML_ERR_INVALID, "%s", bad.c_str());
    }
    const size_t kk = (size_t)ctx->k * ctx->ks;
    dev_release(ctx, &ctx->d_P, (size_t)ctx->C * ctx->N * kk);   // the batch goes: the sweeps no longer read it
    PML_TRY(arm_pij_wide_list(ctx));   // (the LDS attribute of the build kernel: not inside a stream capture)
    int status = dev_alloc(ctx, &ctx->d_pij_window, (size_t)ctx->C * (size_t)B * kk);
    for (int i = 0; i < 2 && status == PML_OK; ++i) {
        status = put(ctx, &ctx->d_win_branches[i], W[i].branches);
        if (status == PML_OK) status = put(ctx, &ctx->d_win_slot[i], W[i].slot);
        ctx->win_branches[i].swap(W[i].branches);
    }
    for (const PmlWindowStep& w : W[1].steps)
        if (w.launch.op == OP_LEVEL && w.launch.list == L_TD_PLAIN && w.launch.count > 0) ctx->win_td_runs.push_back(w);
    ctx->pij_window = B;
    const hipError_t e = hipStreamSynchronize(ctx->stream);   // (the host tables go out of scope)
    if (status != PML_OK || e != hipSuccess) {
        window_drop(ctx);
        return status != PML_OK ? status : fail(PML_ERR_HIP, "upload of the window's tables failed: %s", hipGetErrorString(e));
    }
    return PML_OK;
}

// (NO_MFMA / NO_PIJ_WIDE: the batch is then built by the one-thread-per-entry kernel, whose sums associate differently from the
// matrix-core kernel the window is built with -- a window would not leave the batch's bits, so there is none under them)
static bool window_eligible(const pml_ctx* ctx) {
    return ctx->kind == PML_MODEL_EIGEN && ctx->k > 32 && ctx->k <= PML_MAX_STATES_MATRIX && !ctx->tune.on(T_NO_MFMA) &&
           !ctx->tune.on(T_NO_PIJ_WIDE);
}

// PASTML_HIP_PIJ_WINDOW (branches; 0: the batch): applied where a sweep is submitted, once per value -- the model kind and the
// columns are known there.  It is raised to the largest fan-out and capped at the number of nodes; contexts the window is not
// for (F81, HKY, k <= 32) ignore it.  Not set: what pml_pij_window_set said stands.
PML_INTERNAL int window_from_tunable(pml_ctx* ctx) {
    // (a switch set after the window took away what the window is built with: back to the batch)
    if (ctx->pij_window > 0 && !window_eligible(ctx)) PML_TRY(window_set(ctx, 0));
    if (!ctx->tune.on(T_PIJ_WINDOW)) return PML_OK;
    const long long want = ctx->tune.get(T_PIJ_WINDOW, 0);
    if (want == ctx->pij_window_tuned) return PML_OK;
    ctx->pij_window_tuned = want;
    if (!window_eligible(ctx) || want < 0) return PML_OK;
    return window_set(ctx, want == 0 ? 0 : std::max<long long>(want, pml_window_max_fanout(ctx->forest)));
}

int pml_pij_window_set(pml_ctx* ctx, long long branches) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    if (branches < 0) return fail(PML_ERR_INVALID, "a window of %lld branches", branches);
    if (branches == 0) return window_set(ctx, 0);
    if (ctx->kind < 0) return fail(PML_ERR_INVALID, "set the model first: the window is for eigen models");
    if (!window_eligible(ctx))
        return fail(PML_ERR_UNSUPPORTED, "the P(t) window is for eigen models with 33 .. %d states whose P(t) is built on the matrix "
                    "cores (this context: model kind %d, k = %d, NO_MFMA %d, NO_PIJ_WIDE %d)", PML_MAX_STATES_MATRIX, ctx->kind, ctx->k,
                    (int)ctx->tune.on(T_NO_MFMA), (int)ctx->tune.on(T_NO_PIJ_WIDE));
    const int fan = pml_window_max_fanout(ctx->forest);
    if (branches < fan)
        return fail(PML_ERR_INVALID, "a window of %lld branches is below the largest fan-out of the forest, %d", branches, fan);
    return window_set(ctx, branches);
}

int pml_pij_window_info(pml_ctx* ctx, long long* branches, long long* window_bytes, long long* batch_bytes) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    const long long kk = (long long)ctx->k * ctx->ks * (long long)sizeof(double);
    if (branches) *branches = ctx->pij_window;
    if (window_bytes) *window_bytes = ctx->d_pij_window ? (long long)ctx->C * ctx->pij_window * kk : 0;
    if (batch_bytes) *batch_bytes = ctx->d_P ? (long long)ctx->C * ctx->N * kk : 0;
    return PML_OK;
}

static int ensure_transition_storage(pml_ctx* ctx) {
    if (ctx->kind != PML_MODEL_F81 && !ctx->d_P)
        PML_TRY(dev_alloc(ctx, &ctx->d_P, (size_t)ctx->C * ctx->N * ctx->k * ctx->ks));
    return PML_OK;
}

// What the entries that read P(t) outside a sweep prepare: the batch of the whole tree -- or, on a context with a window
// (pml_pij_window.h), only the parameters the list build reads: they build their matrices run by run, and no batch is allocated.
static int run_prep(pml_ctx* ctx, bool force, bool bu_sweep);
PML_INTERNAL int consumer_prep(pml_ctx* ctx, bool force) {
    if (!pij_windowed(ctx)) return run_prep(ctx, force, false);
    return params_push(ctx);
}

static int run_prep(pml_ctx* ctx, bool force = false, bool bu_sweep = false) {
    // (callers outside a sweep: pml_pij_batch, pml_marginal_counts, downloads; a sweep's own copy went out, or into the
    // capture, before its first launch: enqueue_bottom_up)
    if (!bu_sweep) PML_TRY(params_push(ctx));
    if (!ctx->results.pij_stale() && !force) return PML_OK;
    const PmlTree t = tree_of(ctx);
    const PmlCols c = cols_of(ctx, bu_sweep);
    const PmlModel m = model_of(ctx);
    PML_TRY(ensure_transition_storage(ctx));
    PML_TRY(prof_begin(ctx));
    if (ctx->kind == PML_MODEL_F81) {
        // columns per thread: as many as still leave a few thousand blocks (the branch length is read once per chunk)
        int cpy = 1;
        const int bx = (ctx->N + PML_BLOCK - 1) / PML_BLOCK;
        while (cpy < 8 && cpy * 2 <= ctx->C && (long long)bx * ((ctx->C + 2 * cpy - 1) / (2 * cpy)) >= 4096) cpy *= 2;
        const int ny = (ctx->C + cpy - 1) / cpy;
        dim3 grid(grid_for(ctx, ctx->N, PML_BLOCK, ny), ny);
        hipLaunchKernelGGL(f81_prep_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, t, c, ctx->d_mu, ctx->d_sf,
                           ctx->d_tau, ctx->d_tauf, state_of(ctx), ctx->C, cpy);
        HIP_TRY(hipGetLastError());
    } else {
        if (ctx->kind == PML_MODEL_HKY) {
            dim3 grid(grid_for(ctx, ctx->N, PML_BLOCK, ctx->C), ctx->C);
            hipLaunchKernelGGL(pij_hky_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, t, c, m, ctx->d_P);
        } else if (ctx->k >= 2 && ctx->k <= PML_EIGJ_STRIDE && ctx->d_AT != nullptr && ctx->d_AinvT != nullptr && (ctx->ks & 1) == 0 &&
                   !ctx->tune.on(T_NO_PIJ_VALU) && (ctx->k < 16 || ctx->tune.on(T_NO_MFMA) || ctx->tune.on(T_PIJ_VALU))) {
            PML_TRY(launch_pij_valu(ctx));   // vector-unit path, pml_launch_eigen_joint.hip
        } else if (ctx->k >= 16 && ctx->k <= 32 && !ctx->tune.on(T_NO_MFMA)) {
            PML_TRY(launch_pij_mfma(ctx));   // FP64 matrix-core path, pml_launch_eigen_mfma.hip
        } else if (ctx->k > 32 && !ctx->tune.on(T_NO_MFMA) && !ctx->tune.on(T_NO_PIJ_WIDE)) {
            PML_TRY(launch_pij_wide(ctx));   // the same beyond 32 states: A^T in LDS slices
        } else {
            const int k = ctx->k;
            size_t lds = ((size_t)2 * k * (k + 1) + k) * sizeof(double);
            int use_lds = 1;
            if (lds > 64 * 1024) {  // default dynamic-LDS limit; larger state spaces read A / Ainv through the caches
                use_lds = 0;
                lds = (size_t)k * sizeof(double);
            }
            int bpb = (ctx->N + 2047) / 2048;
            if (bpb < 16) bpb = 16;
            dim3 grid((ctx->N + bpb - 1) / bpb, ctx->C);
            hipLaunchKernelGGL(pij_eigen_kernel, grid, dim3(PML_BLOCK), lds, ctx->stream, t, c, m, ctx->d_P, bpb, use_lds);
        }
        HIP_TRY(hipGetLastError());
    }
    PML_TRY(prof_end(ctx, 2, 1));
    ctx->results.pij_built();
    return PML_OK;
}

int pml_pij(pml_ctx* ctx, int32_t col, int32_t n_t, const double* ts, double* P_out) {
    PML_TRY(require_model(ctx));
    if (col < 0 || col >= ctx->C) return fail(PML_ERR_INVALID, "column out of range");
    if (n_t <= 0 || !ts || !P_out) return fail(PML_ERR_INVALID, "bad t / output arrays");
    PML_TRY(params_push(ctx));
    const size_t kk = (size_t)ctx->k * ctx->k;
    CallScope mem(ctx->stream, false);
    double *d_t, *d_out;
    PML_TRY(mem.put(&d_t, ts, (size_t)n_t));
    PML_TRY(mem.get(&d_out, kk * n_t));
    const size_t total = kk * n_t;
    dim3 grid((unsigned)std::min<size_t>((total + PML_BLOCK - 1) / PML_BLOCK, 65535));
    hipLaunchKernelGGL(pij_explicit_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, cols_of(ctx), model_of(ctx), col,
                       n_t, d_t, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(P_out, d_out, sizeof(double) * kk * n_t, hipMemcpyDeviceToHost, ctx->stream));
    return mem.finish();
}

int pml_pij_batch(pml_ctx* ctx, double* P_out) {
    PML_TRY(require_model(ctx));
    PML_TRY(run_prep(ctx));
    if (P_out) {
        const size_t kk = (size_t)ctx->k * ctx->k;
        std::vector<double> tmp;   // (matrix models: a column's matrices as the sweeps keep them)
        CallScope mem(ctx->stream, false);
        double* d_out;
        PML_TRY(mem.get(&d_out, kk * ctx->N));
        for (int col = 0; col < ctx->C; ++col) {
            if (ctx->kind == PML_MODEL_F81) {
                // expand the stored e per branch: same arithmetic as the explicit kernel
                const size_t total = kk * ctx->N;
                dim3 grid((unsigned)std::min<size_t>((total + PML_BLOCK - 1) / PML_BLOCK, 65535));
                hipLaunchKernelGGL(pij_explicit_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, cols_of(ctx),
                                   model_of(ctx), col, ctx->N, ctx->d_dist, d_out);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(P_out + (size_t)col * ctx->N * kk, d_out, sizeof(double) * kk * ctx->N,
                                       hipMemcpyDeviceToHost, ctx->stream));
            } else {
                // the matrices the sweeps use, transposed back on the host
                tmp.resize((size_t)ctx->N * ctx->k * ctx->ks);
                HIP_TRY(hipMemcpyAsync(tmp.data(), ctx->d_P + (size_t)col * ctx->N * ctx->k * ctx->ks,
                                       tmp.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                HIP_TRY(hipStreamSynchronize(ctx->stream));
                double* out = P_out + (size_t)col * ctx->N * kk;
                for (int n = 0; n < ctx->N; ++n)
                    for (int i = 0; i < ctx->k; ++i)
                        for (int j = 0; j < ctx->k; ++j)
                            out[(size_t)n * kk + (size_t)i * ctx->k + j] = tmp[((size_t)n * ctx->k + j) * ctx->ks + i];
            }
            PML_TRY(mem.finish());
        }
        rows_to_api_inplace(ctx, P_out, kk, (size_t)ctx->C);
    }
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Everything the planners of the sweeps' launch sequences read of a context (pml_schedule.h): the predicates are
// evaluated here, once per plan.
static PmlSweepTraits sweep_traits(const pml_ctx* ctx) {
    PmlSweepTraits t;
    t.f81 = ctx->kind == PML_MODEL_F81;
    t.eigen_fused = eigen_fused(ctx);
    t.eigen_gemm = eigen_gemm(ctx);
    t.eigen_joint_valu = eigen_joint_valu(ctx);
    t.hky_fused = hky_fused(ctx);
    t.wide_states = wide_states(ctx);
    t.k = ctx->k;
    t.W = ctx->W;
    t.C = ctx->C;
    t.sched_cols = ctx->sched_cols;
    t.n_roots = ctx->n_roots;
    t.n_cherries = ctx->n_cherries;
    t.has_init = ctx->has_init;
    t.fuse = ctx->fuse;
    t.Gf = ctx->cols.Gf;
    t.Gt = ctx->cols.Gt;
    t.bu_wide_lanes = ctx->cols.bu_wide_lanes;
    t.level_lists_sorted = ctx->cols.level_lists_sorted;
    t.single_launch = single_launch_sweeps(ctx);
    t.blocks = block_schedule(ctx);
    t.super = super_sweeps(ctx);
    t.thin = thin_bottom_up(ctx);
    t.deep = deep_top_down(ctx);
    t.narrow_units = (int)ctx->tune.get(T_NARROW_UNITS, 0);
    t.no_td_tail = ctx->tune.on(T_NO_TD_TAIL);
    t.no_eigg_tiers = ctx->tune.on(T_NO_EIGG_TIERS);
    t.no_spin_wait = ctx->tune.on(T_NO_SPIN_WAIT);
    t.waves = PML_WAVES_PER_BLOCK;
    const int ks4 = (ctx->k + 3) / 4;
    t.eig_nb = ks4 % 4 == 0 ? 1 : (ks4 % 2 == 0 ? 2 : 4);   // EigShape::NB (pml_kernels_eigen_mfma.h)
    // (the chained launch is the pipelined kernel's: without the pipeline, the two launches)
    t.td_chain = t.f81 && t.super && ctx->sup.chain_depth >= 0 && !ctx->tune.on(T_NO_TD_CHAIN) && !ctx->tune.on(T_NO_TD_SUPER_PIPE);
    t.bu_chain = t.f81 && t.super && ctx->sup.bu_chain_level >= 0 && !ctx->tune.on(T_NO_BU_CHAIN);   // (the plan asks: marginal sweep)
    return t;
}

static PmlSchedules schedules_of(const pml_ctx* ctx) {
    return {&ctx->blocks, &ctx->thin, &ctx->deep, &ctx->sup, &ctx->eig_tiers, &ctx->bt_tiers, &ctx->bu_level_vec_f,
            &ctx->bu_level_vec, &ctx->td_cherry_prefix};
}

// Puts the launches of a plan on the stream, in order and without host synchronisation (so that they can be captured):
// one call of a launcher per record.  bottom_up: they are a bottom-up sweep's, which looks at the flags of the active
// columns.  The profile brackets open and close where a record's bracket differs from the one before it, and a bracket's
// launches are its records.  (What the launches leave behind: pml_plan_outcome.)
// A context with a window (pml_pij_window.h) issues the windowed sequence: the plan's plain level records cut into runs, each run's
// launch behind the one that builds its branches' matrices into the window; the per-branch pass builds nothing.
static int run_plan(pml_ctx* ctx, const std::vector<PmlLaunch>& whole_plan, bool bottom_up, int is_marginal, bool force_prep) {
    const bool windowed = ctx->pij_window > 0 && ctx->kind == PML_MODEL_EIGEN;
    const int wtab = bottom_up ? 0 : 1;
    const std::vector<PmlWindowStep>* cached = nullptr;
    std::vector<PmlLaunch> cut;
    if (windowed) {
        auto same = [](const PmlLaunch& a, const PmlLaunch& b) {
            return a.op == b.op && a.list == b.list && a.kind == b.kind && a.bracket == b.bracket && a.branch == b.branch &&
                   a.signal == b.signal && a.cherries == b.cherries && a.first == b.first && a.count == b.count && a.arg == b.arg;
        };
        for (const pml_ctx::WindowCut& c : ctx->win_cuts)
            if (c.plan.size() == whole_plan.size() && std::equal(c.plan.begin(), c.plan.end(), whole_plan.begin(), same)) cached = &c.steps;
        if (cached == nullptr) {
            PmlWindowPlan W;
            const std::string bad = pml_plan_pij_window(whole_plan, ctx->forest, ctx->bu_order, ctx->td_parents, ctx->pij_window, W);
            if (!bad.empty()) return fail(PML_ERR_INVALID, "%s", bad.c_str());
            if (!W.branches.empty() && W.branches != ctx->win_branches[wtab])
                return fail(PML_ERR_INVALID, "the sweep's runs are not the ones the window's branch lists were uploaded for");
            if (ctx->win_cuts.size() >= 16) ctx->win_cuts.clear();   // (a handful of plans per context: two sweeps, signalling or not)
            ctx->win_cuts.push_back(pml_ctx::WindowCut{whole_plan, std::move(W.steps)});
            cached = &ctx->win_cuts.back().steps;
        }
        cut.reserve(cached->size());
        for (const PmlWindowStep& w : *cached) cut.push_back(w.launch);
    }
    static const std::vector<PmlWindowStep> no_steps;
    const std::vector<PmlWindowStep>& steps = windowed ? *cached : no_steps;
    const std::vector<PmlLaunch>& plan = windowed ? cut : whole_plan;
    size_t at = 0;
    const pml_ctx::EigenTiers& E = ctx->eig_tiers;
    const pml_ctx::BacktraceTiers& B = ctx->bt_tiers;
    const int* order = bottom_up ? ctx->d_bu_order : nullptr;   // (top-down: the nodes of a depth are a contiguous id range)
    const int* offsets = bottom_up ? ctx->d_bu_offsets : ctx->d_td_offsets;
    const int gemm_mode = bottom_up ? PML_EIGG_BU : PML_EIGG_TD;
    const int eig_mode = !bottom_up ? PML_EIG_TD : (is_marginal ? PML_EIG_BU_MARG : PML_EIG_BU_JOINT);
    int open = PML_NO_BRACKET;
    long long launches = 0;
    for (const PmlLaunch& r : plan) {
        if (ctx->tune.on(T_DEBUG))
            fprintf(stderr, "pml plan: branch %d op %d list %d kind %d first %d count %d arg %d bracket %d signal %d%s\n", r.branch,
                    r.op, r.list, r.kind, r.first, r.count, r.arg, r.bracket, (int)r.signal,
                    r.op != OP_SUPER || r.arg <= 0 ? "" : bottom_up ? " (chained: with the stacked units of level arg - 1)"
                                                                    : " (chained: with the stacked units of depth arg - 1)");
        if (r.bracket != open) {
            if (open != PML_NO_BRACKET) PML_TRY(prof_end(ctx, open, launches));
            if (r.bracket != PML_NO_BRACKET) PML_TRY(prof_begin(ctx));
            open = r.bracket;
            launches = 0;
        }
        ++launches;
        const PmlWindowStep* run = windowed ? &steps[at] : nullptr;
        ++at;
        if (run != nullptr && run->build_count > 0) {
            PML_TRY(launch_pij_wide_list(ctx, ctx->d_pij_window, ctx->pij_window, ctx->d_win_branches[wtab] + run->build_first,
                                         run->build_count));
            ++launches;
        }
        const bool joint = r.kind == EIG_JOINT, gemm = r.kind == EIG_GEMM;   // (of the eigen ops; else the fused matrix-core kernels)
        switch (r.op) {
            case OP_RESET_ERR:
                hipLaunchKernelGGL(reset_err_kernel, dim3((ctx->C + 63) / 64), dim3(64), 0, ctx->stream, ctx->d_err, ctx->C,
                                   r.arg ? ctx->d_tip_rest_count : nullptr);
                HIP_TRY(hipGetLastError());
                break;
            case OP_PREP:   // (brackets itself: other callers run it outside a sweep)
                if (!windowed) PML_TRY(run_prep(ctx, force_prep, true));
                break;
            case OP_LOGLIK:
                // ln L and the error words are written straight into pinned host memory by the last kernel
                hipLaunchKernelGGL(loglik_kernel, dim3((ctx->C + PML_BLOCK - 1) / PML_BLOCK), dim3(PML_BLOCK), 0, ctx->stream,
                                   tree_of(ctx), cols_of(ctx, true), state_of(ctx), ctx->C, is_marginal ? 1 : 0, ctx->h_loglik,
                                   ctx->h_err);
                HIP_TRY(hipGetLastError());
                break;
            case OP_LEVEL:
                PML_TRY(dispatch_sweep(ctx, (SweepKind)r.kind, r.list, r.first, r.count, r.cherries, bottom_up,
                                       windowed && (r.list == L_BU_PLAIN || r.list == L_TD_PLAIN) ? wtab : -1));
                break;
            case OP_ROOTS:
                PML_TRY(dispatch_sweep(ctx, SW_ROOTS, L_NONE, 0, r.count));
                break;
            case OP_LEVELS: {
                // (the fused lists of the whole forest are the launcher's default: it picks the sorted ones where they pay)
                const bool whole = r.list == L_BU_FUSED || r.list == L_TD_FUSED;
                const int do_prep = (bottom_up && r.arg && (ctx->results.pij_stale() || force_prep)) ? 1 : 0;
                PML_TRY(dispatch_small_f81(ctx, bottom_up, r.signal, do_prep, whole ? r.first : 0, r.count,
                                           whole ? nullptr : ctx->d_unit_lists[r.list], whole ? nullptr : ctx->d_list_offsets[r.list] + r.first,
                                           bottom_up ? 0 : r.arg));
                break;
            }
            case OP_BLOCKS:
                PML_TRY(dispatch_blocks_f81(ctx, bottom_up, r.first, r.signal));
                break;
            case OP_SUPER:
                PML_TRY(dispatch_super_f81(ctx, bottom_up, r.arg - 1));
                break;
            case OP_STACK:
                PML_TRY(dispatch_stack_f81(ctx, bottom_up, r.first));
                break;
            case OP_EIG_TIPS:
                if (joint) PML_TRY(launch_eigen_joint_tips(ctx));
                else if (gemm) PML_TRY(launch_eigen_gemm(ctx, PML_EIGG_TIPS, ctx->d_tips, 0, ctx->n_tips));
                else PML_TRY(launch_eigen_tips(ctx, is_marginal ? 0 : 1));
                break;
            case OP_EIG_LEVEL: {
                const int* nodes = order ? order + r.first : nullptr;
                const int first = order ? 0 : r.first;
                if (joint) PML_TRY(launch_eigen_joint(ctx, ctx->d_bu_units + r.first, nullptr, 0, r.count));
                else if (gemm) PML_TRY(launch_eigen_gemm(ctx, gemm_mode, nodes, first, r.count));
                else PML_TRY(launch_eigen_fused(ctx, eig_mode, nodes, first, r.count, 0));
                break;
            }
            case OP_EIG_NARROW:
                if (joint) PML_TRY(launch_eigen_joint(ctx, ctx->d_bu_units, offsets, r.first, r.count));
                else if (gemm) PML_TRY(launch_eigen_gemm_narrow(ctx, gemm_mode, order, offsets, r.first, r.count));
                else PML_TRY(launch_eigen_narrow(ctx, eig_mode, order, offsets, r.first, r.count));
                break;
            case OP_EIG_TIER: {   // thin levels in tiers of subtree blocks (pml_ctx::EigenTiers)
                const pml_ctx::EigenTiers::Tier& T = E.tiers[r.first];
                if (joint) PML_TRY(launch_eigen_joint(ctx, E.d_units, E.d_lv, 0, T.depth, E.d_start + T.first_block, T.n_blocks));
                else PML_TRY(launch_eigen_gemm_narrow(ctx, PML_EIGG_BU, E.d_nodes, E.d_lv, 0, T.depth, E.d_start + T.first_block,
                                                      T.n_blocks));
                break;
            }
            case OP_BT_NARROW:
                hipLaunchKernelGGL(joint_backtrace_narrow_kernel, dim3(1, ctx->C), dim3(PML_BLOCK), 0, ctx->stream,
                                   tree_of(ctx), cols_of(ctx), state_of(ctx), ctx->d_td_offsets, r.first, r.count);
                HIP_TRY(hipGetLastError());
                break;
            case OP_BT_TIER: {
                const pml_ctx::BacktraceTiers::Tier& T = B.tiers[r.first];
                hipLaunchKernelGGL(joint_backtrace_blocks_kernel, dim3(T.n_blocks, ctx->C), dim3(PML_BLOCK), 0, ctx->stream,
                                   tree_of(ctx), cols_of(ctx), state_of(ctx), B.d_nodes, B.d_lv, B.d_start + T.first_block,
                                   T.depth);
                HIP_TRY(hipGetLastError());
                break;
            }
            case OP_BT_LEVEL: {
                dim3 grid(grid_for(ctx, r.count, PML_BLOCK, ctx->C), ctx->C);
                hipLaunchKernelGGL(joint_backtrace_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, tree_of(ctx), cols_of(ctx),
                                   state_of(ctx), r.first, r.first + r.count);
                HIP_TRY(hipGetLastError());
                break;
            }
            default:
                return fail(PML_ERR_INVALID, "unknown launch op %d", r.op);
        }
    }
    if (open != PML_NO_BRACKET) PML_TRY(prof_end(ctx, open, launches));
    return PML_OK;
}

// Everything a bottom-up sweep puts on the stream, without host synchronisation (so that it can be captured), as
// pml_plan_bottom_up lists it.
static int enqueue_bottom_up(pml_ctx* ctx, int is_marginal, bool force_prep, PmlCapture capture, PmlSweepOutcome* outcome) {
    const std::vector<PmlLaunch> plan = pml_plan_bottom_up(ctx->forest, schedules_of(ctx), sweep_traits(ctx), is_marginal != 0);
    *outcome = pml_plan_outcome(plan);
    PML_TRY(params_push(ctx, capture, outcome));  // what the last model update left in the pinned mirror (part of the graph when captured)
    return run_plan(ctx, plan, true, is_marginal, force_prep);
}

// Captures enqueue's stream work once and replays it afterwards; outcome: of what now runs on the stream, captured just
// now or replayed.  capture: CAP_PASS -- the stream is being captured already, the work becomes part of that graph.
using PmlEnqueue = std::function<int(PmlCapture, PmlSweepOutcome*)>;
static int run_captured(pml_ctx* ctx, pml_ctx::GraphSlot& slot, PmlCapture capture, const PmlEnqueue& enqueue,
                        PmlSweepOutcome* outcome) {
    if (capture == CAP_PASS) return enqueue(CAP_PASS, outcome);
    if (slot.exec && slot.has_init != ctx->has_init) drop_graph(slot);
    if (!slot.exec) {
        HIP_TRY(hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
        slot.outcome = {};
        const int status = enqueue(CAP_OWN, &slot.outcome);
        hipGraph_t graph = nullptr;
        const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
        if (status != PML_OK) {
            if (graph) (void)hipGraphDestroy(graph);
            return status;
        }
        if (e != hipSuccess || !graph) return fail(PML_ERR_HIP, "stream capture failed: %s", hipGetErrorString(e));
        hipGraphExec_t exec = nullptr;
        const hipError_t e2 = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        if (e2 != hipSuccess) {
            (void)hipGraphDestroy(graph);
            return fail(PML_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e2));
        }
        slot.graph = graph;
        slot.exec = exec;
        slot.has_init = ctx->has_init;
    }
    HIP_TRY(hipGraphLaunch(slot.exec, ctx->stream));
    if (slot.outcome.has_params) ctx->params_dirty = false;
    *outcome = slot.outcome;
    return PML_OK;
}

// Which columns the next bottom-up sweep computes (nullptr: all).  The flags travel with the parameter block (params_push:
// inside the captured sweep when it is replayed), so they are written while no sweep is in flight, like the parameters.
static void set_active_columns(pml_ctx* ctx, const uint8_t* active) {
    if (!ctx->h_params) return;
    double* flags = ctx->h_params + ctx->cols.params.active;
    if (active == nullptr && !ctx->active_partial) {  // (all ones already)
        ctx->n_active = ctx->C;
        return;
    }
    bool partial = false, changed = false;
    int n = 0;
    for (int i = 0; i < ctx->C; ++i) {
        const double v = (active == nullptr || active[i]) ? 1.0 : 0.0;
        changed = changed || flags[i] != v;
        partial = partial || v == 0.0;
        n += v != 0.0;
        flags[i] = v;
    }
    ctx->active_partial = partial;
    ctx->n_active = n;
    if (changed) ctx->params_dirty = true;
}

// the sweep never reads the batch of P(t): the fused eigen sweeps build it in registers, the two-GEMM sweeps never form it
static bool sweep_without_p(const pml_ctx* ctx, int is_marginal) {
    return eigen_fused(ctx) || (is_marginal && eigen_gemm(ctx)) || (!is_marginal && eigen_joint_valu(ctx)) || hky_fused(ctx);
}

// what a bottom-up sweep leaves behind (a replayed pml_marginal_pass runs no submit_bottom_up)
static void note_bottom_up(pml_ctx* ctx, int is_marginal, const PmlSweepOutcome& outcome) {
    const bool ran_batch = !sweep_without_p(ctx, is_marginal) && ctx->pij_window == 0;
    ctx->results.bottom_up_submitted(is_marginal != 0, ctx->kind == PML_MODEL_F81, ctx->n_cherries > 0, super_sweeps(ctx), ran_batch,
                                     ctx->active_partial, outcome.fused_joint);
}

// Waits for what was submitted last (a bottom-up sweep, a marginal pass).  Where its last launch raises the pinned word
// (pml_signal_done) the host spins on that word -- the results lie in pinned memory behind it -- instead of asking the
// runtime, which notices the end of a short launch sequence ~4 us later (scripts/ub/syncwait.hip); after 2 ms, or for
// anything else, it is hipStreamSynchronize.  Everything queued afterwards is ordered behind the sweep by the stream as
// before.  idle: the caller needs the stream idle, not just the results (the word is raised before its kernel has ended:
// blocking copies on the NULL stream, the generation the next submission reads).
PML_INTERNAL int wait_pending(pml_ctx* ctx, bool idle) {
    const bool spin = ctx->pending.spin && !idle && ctx->h_done;
    ctx->pending.spin = false;
    if (spin) {
        const u64* flag = ctx->h_done;
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spins = 0;; ++spins) {
            // (acquire: the results the host reads next were written before the word was raised)
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) >= ctx->pending.expect) return PML_OK;
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if ((spins & 1023u) == 1023u &&
                std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2))
                break;
        }
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PML_OK;
}

// Opens a submission: the generation the completion word shows before it.  (A sweep submitted and never collected is
// waited for first: the word is read on an idle stream.)
static int generation_before(pml_ctx* ctx, u64* generation) {
    if (ctx->pending.spin) PML_TRY(wait_pending(ctx, true));
    *generation = ctx->h_done ? *reinterpret_cast<volatile u64*>(ctx->h_done) : 0;
    return PML_OK;
}

// puts a bottom-up sweep on the stream (no host synchronisation).  may_spin: whoever waits for the sweep reads nothing but
// what lies behind its completion word (wait_pending); capture: CAP_NONE, or CAP_PASS inside the graph of a marginal pass
static int submit_bottom_up(pml_ctx* ctx, int is_marginal, const uint8_t* active, bool may_spin, PmlCapture capture,
                            PmlSweepOutcome* outcome) {
    set_active_columns(ctx, active);
    if (capture == CAP_NONE) PML_TRY(window_from_tunable(ctx));
    u64 generation = 0;
    PML_TRY(generation_before(ctx, &generation));
    // A sweep of a few columns of a context of many is scheduled as a context of few would be (the workgroups of the
    // other columns return at once): subtree blocks instead of one workgroup per column walking every level, the
    // completion word -- HIV1C tree, 6 of 246 binary columns: 0.15 -> 0.10 ms per sweep.  Two schedules, two captured
    // sequences: all the columns' (sched_cols = C) and a few columns' (sched_cols = 32).
    bool few = ctx->active_partial && ctx->n_active <= 32 && ctx->C > 32 && is_marginal && ctx->kind == PML_MODEL_F81;
    if (few) {  // (only where the few-column schedule is the subtree blocks: never from one launch to one per level)
        ctx->sched_cols = 32;
        few = !single_launch_sweeps(ctx) && block_schedule(ctx);
        ctx->sched_cols = ctx->C;
    }
    struct Sched {
        pml_ctx* c;
        Sched(pml_ctx* x, int cols) : c(x) { c->sched_cols = cols; }
        ~Sched() { c->sched_cols = c->C; }
    } sched(ctx, few ? 32 : ctx->C);
    const bool small_path = single_launch_sweeps(ctx) && is_marginal && ctx->kind == PML_MODEL_F81;
    const size_t CN = (size_t)ctx->C * ctx->N;
    if (!is_marginal && !ctx->d_J) {
        PML_TRY(dev_alloc(ctx, &ctx->d_J, CN * ctx->ks * (ctx->k > 256 ? 2 : 1)));
        PML_TRY(dev_alloc(ctx, &ctx->d_js, CN));
    }
    if (eigen_fused(ctx) || eigen_gemm(ctx) || eigen_joint_valu(ctx)) {
        if (!ctx->d_msg) PML_TRY(dev_alloc(ctx, &ctx->d_msg, CN * ctx->ks));
    }
    if (!is_marginal && eigen_joint_valu(ctx) && !ctx->d_tip_rest) {
        PML_TRY(dev_alloc(ctx, &ctx->d_tip_rest, (size_t)ctx->C * std::max(1, ctx->n_tips)));
        PML_TRY(dev_alloc(ctx, &ctx->d_tip_rest_count, (size_t)ctx->C));
    }
    if (!sweep_without_p(ctx, is_marginal) && ctx->pij_window == 0) PML_TRY(ensure_transition_storage(ctx));
    ctx->results.no_results();   // (from here on the buffers are being overwritten, whether every launch goes through or not)
    // mid-size forests: the level launches are latency-bound, replay them as one hipGraph
    const int n_launches = small_path ? 1 : (is_marginal && ctx->kind == PML_MODEL_F81 ? (int)ctx->forest.bu_offsets_f.size() - 1
                                                                                          : ctx->n_bu_levels);
    if (ctx->graphs && !ctx->profile && n_launches >= 4) {  // (the block schedule's few launches replay as a graph too)
        pml_ctx::GraphSlot& graph = few ? ctx->bu_graph_few : ctx->bu_graph[is_marginal ? 1 : 0];
        PML_TRY(run_captured(ctx, graph, capture, [&](PmlCapture c, PmlSweepOutcome* o) -> int { return enqueue_bottom_up(ctx, is_marginal, true, c, o); },
                             outcome));
    } else {
        // (inside the capture of a whole marginal pass the per-branch pass must be part of the graph)
        PML_TRY(enqueue_bottom_up(ctx, is_marginal, capture == CAP_PASS, capture, outcome));
    }
    ctx->pending = {generation + 1, outcome->final_signals && may_spin && capture == CAP_NONE && !ctx->tune.on(T_NO_SPIN_WAIT)};
    note_bottom_up(ctx, is_marginal, *outcome);
    return PML_OK;
}
// a sweep of its own, waited for by wait_pending (pml_bottom_up, pml_bottom_up_submit / _collect)
static int submit_bottom_up(pml_ctx* ctx, int is_marginal, const uint8_t* active = nullptr) {
    PmlSweepOutcome outcome;
    return submit_bottom_up(ctx, is_marginal, active, true, CAP_NONE, &outcome);
}

// after the stream has been synchronised: log-likelihoods and zero-likelihood reports of the last sweep
static int collect_bottom_up(pml_ctx* ctx, int is_marginal, double* loglik_out, int32_t* err_parent, int32_t* err_child) {
    memcpy(loglik_out, ctx->h_loglik, sizeof(double) * ctx->C);
    const u64* err = ctx->h_err;
    int status = PML_OK;
    const double* flags = ctx->h_params + ctx->cols.params.active;
    for (int c = 0; c < ctx->C; ++c) {
        int ep = -1, ec = -1;
        if (err[c] != ~0ull && flags[c] != 0.0) {  // (a column that sat the sweep out reports nothing)
            ec = (int)(err[c] & 0xffffffffull);
            ep = api_id(ctx, ctx->forest.parent[ec]);
            ec = api_id(ctx, ec);
            if (status == PML_OK)
                status = fail(PML_ZERO_LIKELIHOOD, "zero likelihood in column %d between parent %d and child %d", c, ep, ec);
        }
        if (err_parent) err_parent[c] = ep;
        if (err_child) err_child[c] = ec;
    }
    if (status == PML_OK) ctx->results.bottom_up_collected(is_marginal != 0);
    return status;
}

int pml_bottom_up(pml_ctx* ctx, int is_marginal, double* loglik_out, int32_t* err_parent, int32_t* err_child) {
    PML_TRY(require_model(ctx));
    if (!loglik_out) return fail(PML_ERR_INVALID, "loglik_out is NULL");
    PML_TRY(submit_bottom_up(ctx, is_marginal));
    PML_TRY(wait_pending(ctx));
    return collect_bottom_up(ctx, is_marginal, loglik_out, err_parent, err_child);
}

int pml_bottom_up_submit(pml_ctx* ctx, int is_marginal) {
    PML_TRY(require_model(ctx));
    return submit_bottom_up(ctx, is_marginal);
}

int pml_bottom_up_submit_columns(pml_ctx* ctx, int is_marginal, const uint8_t* active) {
    PML_TRY(require_model(ctx));
    if (!is_marginal || ctx->kind != PML_MODEL_F81) active = nullptr;  // (only the F81 marginal kernels look at the flags)
    return submit_bottom_up(ctx, is_marginal, active);
}

int pml_bottom_up_collect(pml_ctx* ctx, int is_marginal, double* loglik_out, int32_t* err_parent, int32_t* err_child) {
    if (!ctx || ctx->C == 0) return fail(PML_ERR_INVALID, "allocate the columns first");
    if (!loglik_out) return fail(PML_ERR_INVALID, "loglik_out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    PML_TRY(wait_pending(ctx));
    return collect_bottom_up(ctx, is_marginal, loglik_out, err_parent, err_child);
}

// The observed tips' rows and a top-down sweep about to go on the stream (before its capture or replay, never inside one).
// Where the record says that the rows stand (PmlResults::tip_rows_kept) the F81 kernels of one mask word leave their stores
// out: the word travels at the end of the parameter block, whose copy is part of a captured sweep, so a replayed graph reads the
// word of the day as it reads the flags of the active columns.  PASTML_HIP_NO_KEEP_TIP_ROWS: every sweep writes every row.  The
// bad-tip word is cleared here and read by end_top_down.
static bool tip_rows_skipped(const pml_ctx* ctx) { return ctx->h_params != nullptr && ctx->h_params[ctx->cols.params.keep_tips] != 0.0; }
static void begin_top_down(pml_ctx* ctx) {
    const bool skip = ctx->results.tip_rows_kept() && !ctx->tune.on(T_NO_KEEP_TIP_ROWS) && !ctx->implicit_tips &&
                      ctx->kind == PML_MODEL_F81 && ctx->W == 1;
    if (skip != tip_rows_skipped(ctx)) {
        ctx->h_params[ctx->cols.params.keep_tips] = skip ? 1.0 : 0.0;
        ctx->params_dirty = true;
    }
    *reinterpret_cast<volatile u64*>(ctx->h_bad_tip) = 0;
}
// behind the wait every top-down entry ends in: the sweep's rows stand unless it wrote NaNs over one of them
static void end_top_down(pml_ctx* ctx) { ctx->results.top_down_waited(__atomic_load_n(ctx->h_bad_tip, __ATOMIC_ACQUIRE) != 0); }

// what a top-down sweep leaves behind (a replayed pml_marginal_pass runs no run_top_down)
static void note_top_down(pml_ctx* ctx) {
    const bool f81_one_word = ctx->kind == PML_MODEL_F81 && ctx->W == 1;
    if (ctx->tune.on(T_DEBUG))
        fprintf(stderr, "pml plan: top-down sweep, observed tips' rows %s\n",
                !f81_one_word ? "written (not the F81 kernels of one mask word)" : state_of(ctx).implicit_tips ? "implicit"
                : tip_rows_skipped(ctx) ? "kept" : "written");
    ctx->results.top_down_submitted(ctx->kind != PML_MODEL_F81 || ctx->keep_td, state_of(ctx).implicit_tips, f81_one_word);
}

// the top-down launches (shared by pml_top_down_marginals and the lazy TD materialisation of pml_download), as
// pml_plan_top_down lists them; wants_signal: the caller waits on the completion word of the last launch
static int run_top_down(pml_ctx* ctx, bool wants_signal = false, PmlCapture capture = CAP_NONE, PmlSweepOutcome* outcome = nullptr) {
    const size_t CN = (size_t)ctx->C * ctx->N;
    const bool td_stored = ctx->kind != PML_MODEL_F81 || ctx->keep_td;
    if (td_stored && !ctx->d_td) {
        PML_TRY(dev_alloc(ctx, &ctx->d_td, CN * ctx->ks));
        PML_TRY(dev_alloc(ctx, &ctx->d_te, CN));
    }
    if (!ctx->d_post) {
        PML_TRY(dev_alloc(ctx, &ctx->d_post, CN * ctx->ks));
        PML_TRY(dev_alloc(ctx, &ctx->d_lhsum, CN));
        PML_TRY(dev_alloc(ctx, &ctx->d_lhe, CN));
    }
    const bool td_small = single_launch_sweeps(ctx) && ctx->kind == PML_MODEL_F81;
    if (capture != CAP_PASS) {   // (a captured pass: pml_marginal_pass did this before the capture began)
        begin_top_down(ctx);
        PML_TRY(params_push(ctx));   // only where the word changed: a sweep of its own holds no copy of the block
    }
    auto enqueue = [&](PmlCapture, PmlSweepOutcome* o) -> int {   // (a replayed graph plans nothing)
        const std::vector<PmlLaunch> plan = pml_plan_top_down(ctx->forest, schedules_of(ctx), sweep_traits(ctx), wants_signal);
        *o = pml_plan_outcome(plan);
        return run_plan(ctx, plan, false, 1, false);
    };
    PmlSweepOutcome done;
    if (ctx->graphs && !ctx->profile && !td_small && ctx->n_td_levels >= 4) {
        PML_TRY(run_captured(ctx, ctx->td_graph, capture, enqueue, &done));
    } else {
        PML_TRY(enqueue(capture, &done));
    }
    if (outcome) *outcome = done;
    note_top_down(ctx);
    return PML_OK;
}

// For inspection (pml_download of the TD buffers): every non-root node gets its top-down vector.  F81 family: the
// sweep did not write its TD vectors, it is repeated with the stores switched on (same arithmetic); then the vectors of
// the nodes no sweep stores (tips; fused cherries) are filled in level by level (td_fill_kernel).
static int materialize_td(pml_ctx* ctx) {
    if (ctx->results.td_vectors_missing()) {
        // one sweep with the stores on; the option itself stays as the caller set it (a pooled ctx must not keep
        // paying for TD stores because somebody once looked at them)
        const bool was = ctx->keep_td;
        drop_graph(ctx->td_graph);
        drop_graph(ctx->mp_graph);
        ctx->keep_td = true;
        const int status = run_top_down(ctx);
        ctx->keep_td = was;
        if (!was) {
            drop_graph(ctx->td_graph);
            drop_graph(ctx->mp_graph);
        }
        const hipError_t waited = status == PML_OK ? hipStreamSynchronize(ctx->stream) : hipSuccess;
        if (status != PML_OK || waited != hipSuccess) ctx->results.tip_rows_unknown();
        PML_TRY(status);
        HIP_TRY(waited);
        end_top_down(ctx);
    }
    if (ctx->results.td_fill_missing()) {
        const bool f81 = ctx->kind == PML_MODEL_F81;
        if (f81) {
            PML_TRY(materialize_cherries(ctx));  // the cherries' bottom-up vectors
        } else {
            PML_TRY(run_prep(ctx, ctx->d_P == nullptr || eigen_fused(ctx) || eigen_gemm(ctx)));  // P(t) of every branch in HBM
        }
        PmlState st = state_of(ctx);
        st.td = ctx->d_td;  // state_of hides them when the option is off
        st.te = ctx->d_te;
        for (int d = 1; d < ctx->n_td_levels; ++d) {
            const int a = ctx->forest.td_offsets[d], b = ctx->forest.td_offsets[d + 1];
            if (b <= a) continue;
            dim3 grid(grid_for(ctx, b - a, PML_WAVES_PER_BLOCK, ctx->C), ctx->C);
            hipLaunchKernelGGL(td_fill_kernel, grid, dim3(PML_BLOCK), 0, ctx->stream, tree_of(ctx, f81), cols_of(ctx), st,
                               f81 ? nullptr : ctx->d_P, f81 ? 1 : 0, a, b);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->results.td_fill_written();
    }
    return PML_OK;
}

// copies of the marginal results the caller asked for (stream-ordered behind the sweep), then one synchronisation
static int fetch_marginals(pml_ctx* ctx, double* posterior_out, double* lh_sum_out, double* lh_sf_out) {
    const size_t CN = (size_t)ctx->C * ctx->N;
    if (posterior_out) {
        PML_TRY(materialize_tip_posteriors(ctx));
        PML_TRY(fetch_rows(ctx, ctx->d_post, (size_t)ctx->ks, (size_t)ctx->k, (size_t)ctx->C, posterior_out));
    }
    PML_TRY(fetch_rows(ctx, ctx->d_lhsum, 1, 1, (size_t)ctx->C, lh_sum_out));
    // (the exponents arrive in the output array itself -- same width -- and are converted in place)
    PML_TRY(fetch_rows(ctx, ctx->d_lhe, 1, 1, (size_t)ctx->C, reinterpret_cast<i64*>(lh_sf_out)));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (lh_sf_out) {
        const double l2 = std::log10(2.0);
        const i64* e = reinterpret_cast<const i64*>(lh_sf_out);
        for (size_t i = 0; i < CN; ++i) lh_sf_out[i] = -(double)e[i] * l2;
    }
    return PML_OK;
}

int pml_top_down_marginals(pml_ctx* ctx, double* posterior_out, double* lh_sum_out, double* lh_sf_out) {
    PML_TRY(require_model(ctx));
    if (!ctx->results.has_marginal()) return fail(PML_ERR_INVALID, "pml_top_down_marginals needs a successful marginal pml_bottom_up first");
    int status = run_top_down(ctx);
    if (status == PML_OK) status = fetch_marginals(ctx, posterior_out, lh_sum_out, lh_sf_out);   // synchronises
    if (status == PML_OK) end_top_down(ctx);
    else ctx->results.tip_rows_unknown();
    return status;
}

static int marginal_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child, double* posterior_out,
                         double* lh_sum_out, double* lh_sf_out);

int pml_marginal_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child, double* posterior_out,
                      double* lh_sum_out, double* lh_sf_out) {
    PML_TRY(require_model(ctx));
    if (!loglik_out) return fail(PML_ERR_INVALID, "loglik_out is NULL");
    const int status = marginal_pass(ctx, loglik_out, err_parent, err_child, posterior_out, lh_sum_out, lh_sf_out);
    if (status != PML_OK) ctx->results.tip_rows_unknown();   // a zero likelihood, a HIP failure: whatever the sweep wrote
    return status;
}

static int marginal_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child, double* posterior_out,
                         double* lh_sum_out, double* lh_sf_out) {
    // both sweeps go on the stream before the host looks at anything: the top-down sweep does not wait for a round trip.
    // Latency-bound forests (the sweeps replay as hipGraphs): ONE graph holds both sweeps -- one launch call, no gap
    // between the last bottom-up kernel and the first top-down one.  (F81 family, once the buffers of a top-down sweep
    // exist: nothing may be allocated while a stream is captured.)
    const bool td_small = single_launch_sweeps(ctx) && ctx->kind == PML_MODEL_F81;
    const int bu_launches = td_small ? 1 : (int)ctx->forest.bu_offsets_f.size() - 1;
    const bool one_graph = ctx->graphs && !ctx->profile && ctx->kind == PML_MODEL_F81 && ctx->d_post != nullptr &&
                           (!ctx->keep_td || ctx->d_td != nullptr) &&
                           (bu_launches >= 4 || (!td_small && ctx->n_td_levels >= 4));
    // Where the pass ends in a multi-level kernel and has few columns, that kernel says when it is done (pml_signal_done)
    // and the wait at the end of this call is a spin on the word it raises (wait_pending) -- as for a bottom-up sweep.
    // The word counts the signalling launches (the bottom-up sweep's last one may be one too).
    u64 generation = 0;
    PML_TRY(generation_before(ctx, &generation));
    set_active_columns(ctx, nullptr);  // (the replayed pass does not go through submit_bottom_up)
    begin_top_down(ctx);               // (nor through run_top_down; the word goes out with the bottom-up sweep's copy of the block)
    PmlSweepOutcome pass;
    if (one_graph) {
        PML_TRY(run_captured(ctx, ctx->mp_graph, CAP_NONE, [&](PmlCapture, PmlSweepOutcome* o) -> int {
            PmlSweepOutcome td;
            PML_TRY(submit_bottom_up(ctx, 1, nullptr, false, CAP_PASS, o));
            PML_TRY(run_top_down(ctx, true, CAP_PASS, &td));
            o->then(td);
            return PML_OK;
        }, &pass));
        // the bookkeeping of submit_bottom_up / run_top_down (a replay runs neither)
        note_bottom_up(ctx, 1, pass);
        note_top_down(ctx);
    } else {
        PmlSweepOutcome td;
        PML_TRY(submit_bottom_up(ctx, 1, nullptr, false, CAP_NONE, &pass));  // (this call waits for the whole pass)
        PML_TRY(run_top_down(ctx, td_small, CAP_NONE, &td));  // (the single launch is enqueued afresh every time; level sweeps may replay a graph)
        pass.then(td);
    }
    ctx->pending = {generation + (u64)pass.n_signals, pass.final_signals && ctx->comm == nullptr && !posterior_out && !lh_sum_out &&
                                                          !lh_sf_out && !ctx->tune.on(T_NO_SPIN_WAIT)};
    // a communicator is attached: the one collective of the path goes on the stream right here, behind the sweeps --
    // the rank's sum formed on the device from the values the sweep left in pinned memory, all-reduced over RCCL, copied
    // back; the single wait of this call (fetch_marginals) covers it.  pml_loglik_total hands the result out.
    if (ctx->comm != nullptr) {
        PmlComm* cm = ctx->comm;
        hipLaunchKernelGGL(sum_loglik_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->h_loglik, ctx->C, cm->d_total);
        HIP_TRY(hipGetLastError());
        if (cm->comm) {
            PmlRccl* r = pml_rccl();
            const ncclResult_t e = r->AllReduce(cm->d_total, cm->d_total, 1, ncclDouble, ncclSum, cm->comm, ctx->stream);
            if (e != ncclSuccess) return fail(PML_ERR_HIP, "ncclAllReduce failed: %s", r->GetErrorString(e));
        }
        HIP_TRY(hipMemcpyAsync(cm->h_total, cm->d_total, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        cm->total_fresh = true;
    }
    int fetched = PML_OK;
    if (ctx->pending.spin) {
        fetched = wait_pending(ctx);  // (nothing to copy: the spin on the last launch's word, or the stream)
    } else {
        fetched = fetch_marginals(ctx, posterior_out, lh_sum_out, lh_sf_out);  // synchronises
    }
    if (fetched == PML_OK) end_top_down(ctx);   // (the bad-tip word lies behind the completion word, as ln L does)
    const int status = collect_bottom_up(ctx, 1, loglik_out, err_parent, err_child);
    if (status != PML_OK) {
        ctx->results.no_results();  // a column without likelihood: its top-down results mean nothing
        return status;
    }
    return fetched;
}

// the back-trace launches (no host synchronisation), as pml_plan_backtrace lists them
static int submit_joint_backtrace(pml_ctx* ctx) {
    int head = 0;
    const std::vector<PmlLaunch> plan = pml_plan_backtrace(ctx->forest, schedules_of(ctx), sweep_traits(ctx), &head);
    auto enqueue = [&](PmlCapture, PmlSweepOutcome* o) -> int {
        *o = pml_plan_outcome(plan);
        return run_plan(ctx, plan, false, 0, false);
    };
    PmlSweepOutcome done;   // (no launch of the back-trace signals: fetch_joint_states waits on the stream)
    if (ctx->graphs && !ctx->profile && ctx->n_td_levels - head >= 4) return run_captured(ctx, ctx->bt_graph, CAP_NONE, enqueue, &done);
    return enqueue(CAP_NONE, &done);
}

static int fetch_joint_states(pml_ctx* ctx, int32_t* joint_state_out) {
    ctx->results.joint_states_fetched();
    PML_TRY(fetch_rows(ctx, ctx->d_js, 1, 1, (size_t)ctx->C, joint_state_out));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PML_OK;
}

int pml_joint_backtrace(pml_ctx* ctx, int32_t* joint_state_out) {
    PML_TRY(require_model(ctx));
    if (!ctx->results.has_joint()) return fail(PML_ERR_INVALID, "pml_joint_backtrace needs a successful joint pml_bottom_up first");
    PML_TRY(submit_joint_backtrace(ctx));
    return fetch_joint_states(ctx, joint_state_out);
}

int pml_joint_pass(pml_ctx* ctx, double* loglik_out, int32_t* err_parent, int32_t* err_child, int32_t* joint_state_out) {
    PML_TRY(require_model(ctx));
    if (!loglik_out) return fail(PML_ERR_INVALID, "loglik_out is NULL");
    // joint sweep and back-trace submitted together: one host round trip
    PmlSweepOutcome sweep;
    PML_TRY(submit_bottom_up(ctx, 0, nullptr, false, CAP_NONE, &sweep));  // (fetch_joint_states waits for both)
    PML_TRY(submit_joint_backtrace(ctx));
    const int fetched = fetch_joint_states(ctx, joint_state_out);  // synchronises
    const int status = collect_bottom_up(ctx, 0, loglik_out, err_parent, err_child);
    if (status != PML_OK) {
        ctx->results.no_results();
        return status;
    }
    return fetched;
}

// Maximum parsimony of n_cols characters on the uploaded forest (pml_launch_parsimony.hip).  Needs the tree only: no columns,
// no model, no likelihood vectors -- the scratch of the call is freed before it returns.
int pml_parsimony(pml_ctx* ctx, int32_t n_cols, int32_t k, const uint64_t* given, int methods, uint64_t* sets_out,
                  int64_t* steps_out, int64_t* size_hist_out) {
    if (!ctx || ctx->N == 0) return fail(PML_ERR_INVALID, "upload the tree first");
    if (n_cols <= 0) return fail(PML_ERR_INVALID, "n_cols must be positive");
    if (k <= 0) return fail(PML_ERR_INVALID, "k must be positive");
    if (k > PML_MAX_STATES) return fail(PML_ERR_UNSUPPORTED, "k = %d states; at most %d are supported", k, PML_MAX_STATES);
    if (methods <= 0 || methods > 7) return fail(PML_ERR_INVALID, "methods must be a combination of PML_PARS_ACCTRAN / _DOWNPASS / _DELTRAN");
    if (!given || !sets_out || !steps_out || !size_hist_out) return fail(PML_ERR_INVALID, "NULL array");
    return launch_parsimony(ctx, n_cols, k, (const u64*)given, methods, (u64*)sets_out, (i64*)steps_out, (i64*)size_hist_out);
}

int pml_parsimony_info(pml_ctx* ctx, int64_t* launches, double* passes_ms) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (launches) *launches = ctx->pars_launches;
    if (passes_ms) *passes_ms = ctx->pars_ms;
    return PML_OK;
}

// Vertical collapse of the uploaded forest by equal state sets (pml_launch_compress.hip).  Needs the tree only; the scratch of
// the call is freed before it returns.
int pml_compress_vertical(pml_ctx* ctx, int32_t n_cols, int32_t W, const uint64_t* sets, const uint8_t* is_polytomy,
                          int32_t* top_out, int32_t* tips_inside_out, int32_t* internal_inside_out, int32_t* parent_vertex_out) {
    if (!ctx || ctx->N == 0) return fail(PML_ERR_INVALID, "upload the tree first");
    if (n_cols <= 0) return fail(PML_ERR_INVALID, "n_cols must be positive");
    if (W <= 0) return fail(PML_ERR_INVALID, "W must be positive");
    if (W > PML_MAX_STATES / 64) return fail(PML_ERR_UNSUPPORTED, "W = %d words; at most %d are supported", W, PML_MAX_STATES / 64);
    if (!sets || !top_out || !tips_inside_out || !internal_inside_out || !parent_vertex_out)
        return fail(PML_ERR_INVALID, "NULL array");
    return launch_compress(ctx, n_cols, W, (const u64*)sets, is_polytomy, top_out, tips_inside_out, internal_inside_out,
                           parent_vertex_out);
}

int pml_compress_vertical_info(pml_ctx* ctx, double* merged_ms, double* jump_ms, double* counts_ms, int32_t* rounds) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (merged_ms) *merged_ms = ctx->compress_ms[0];
    if (jump_ms) *jump_ms = ctx->compress_ms[1];
    if (counts_ms) *counts_ms = ctx->compress_ms[2];
    if (rounds) *rounds = ctx->compress_rounds;
    return PML_OK;
}

// One pass of the horizontal merging over a forest of vertices given as arrays (pml_launch_compress_horizontal.hip).  The
// context supplies the device and the stream; the uploaded forest is not used.  The scratch of the call is freed before it returns.
int pml_compress_horizontal(pml_ctx* ctx, int32_t n_vertices, int32_t n_cols, int32_t W, const int32_t* parent, const int32_t* rank,
                            const int32_t* bin, const int32_t* width_in, const uint8_t* live_in, const uint64_t* sets,
                            int32_t* into_out, uint8_t* live_out, int32_t* width_out, int32_t* groups_out) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (n_vertices <= 0) return fail(PML_ERR_INVALID, "n_vertices must be positive");
    if (n_cols <= 0) return fail(PML_ERR_INVALID, "n_cols must be positive");
    if (W <= 0) return fail(PML_ERR_INVALID, "W must be positive");
    if (W > PML_MAX_STATES / 64) return fail(PML_ERR_UNSUPPORTED, "W = %d words; at most %d are supported", W, PML_MAX_STATES / 64);
    if (!parent || !rank || !bin || !width_in || !live_in || !sets || !into_out || !live_out || !width_out)
        return fail(PML_ERR_INVALID, "NULL array");
    return launch_compress_horizontal(ctx, n_vertices, n_cols, W, parent, rank, bin, width_in, live_in, (const u64*)sets, into_out,
                                      live_out, width_out, groups_out);
}

int pml_compress_horizontal_info(pml_ctx* ctx, double* states_ms, double* levels_ms, double* down_ms, int32_t* levels,
                                 int64_t* launches, int64_t* table_slots, int32_t* sort_tile) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (states_ms) *states_ms = ctx->hz_ms[0];
    if (levels_ms) *levels_ms = ctx->hz_ms[1];
    if (down_ms) *down_ms = ctx->hz_ms[2];
    if (levels) *levels = ctx->hz_levels;
    if (launches) *launches = ctx->hz_launches;
    if (table_slots) *table_slots = ctx->hz_slots;
    if (sort_tile) *sort_tile = PML_HZ_SORT_TILE;
    return PML_OK;
}

// The trimming of a horizontally merged forest given as arrays (pml_launch_compress_trim.hip).  The context supplies the device
// and the stream; the uploaded forest is not used.  The scratch of the call is freed before it returns.
int pml_compress_trim(pml_ctx* ctx, int32_t n_vertices, int32_t n_cols, int32_t W, const int32_t* parent, const int32_t* tree,
                      const int32_t* n_tips_total, const int32_t* width, const uint64_t* sets, int32_t tip_size_threshold,
                      int32_t n_trees, const uint8_t* trim_tree, double* tsize_out, uint8_t* keep_out, uint8_t* spliced_out,
                      int32_t* new_parent_out, uint8_t* moved_out, double* threshold_out) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (n_vertices <= 0) return fail(PML_ERR_INVALID, "n_vertices must be positive");
    if (n_cols <= 0) return fail(PML_ERR_INVALID, "n_cols must be positive");
    if (n_trees <= 0) return fail(PML_ERR_INVALID, "n_trees must be positive");
    if (W <= 0) return fail(PML_ERR_INVALID, "W must be positive");
    if (W > PML_MAX_STATES / 64) return fail(PML_ERR_UNSUPPORTED, "W = %d words; at most %d are supported", W, PML_MAX_STATES / 64);
    if (tip_size_threshold < 0) return fail(PML_ERR_INVALID, "tip_size_threshold must not be negative");
    if (!parent || !tree || !n_tips_total || !width || !sets || !trim_tree || !tsize_out || !keep_out || !spliced_out ||
        !new_parent_out || !moved_out || !threshold_out)
        return fail(PML_ERR_INVALID, "NULL array");
    return launch_compress_trim(ctx, n_vertices, n_cols, W, parent, tree, n_tips_total, width, (const u64*)sets, tip_size_threshold,
                                n_trees, trim_tree, tsize_out, keep_out, spliced_out, new_parent_out, moved_out, threshold_out);
}

int pml_compress_trim_info(pml_ctx* ctx, double* sizes_ms, double* removal_ms, double* mediators_ms, int32_t* levels, int32_t* rounds,
                           int64_t* launches, int32_t* scan_tile) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (sizes_ms) *sizes_ms = ctx->trim_ms[0];
    if (removal_ms) *removal_ms = ctx->trim_ms[1];
    if (mediators_ms) *mediators_ms = ctx->trim_ms[2];
    if (levels) *levels = ctx->trim_levels;
    if (rounds) *rounds = ctx->trim_rounds;
    if (launches) *launches = ctx->trim_launches;
    if (scan_tile) *scan_tile = PML_TRIM_SCAN_TILE;
    return PML_OK;
}

// The timeline of a compressed forest given as arrays (pml_launch_timeline.hip).  The context supplies the device and the stream;
// the uploaded forest is not used.  The scratch of the call is freed before it returns.
int pml_timeline(pml_ctx* ctx, const pml_timeline_in* in, const pml_timeline_out* out) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (!in || !out) return fail(PML_ERR_INVALID, "NULL argument");
    if (in->n_nodes <= 0) return fail(PML_ERR_INVALID, "n_nodes must be positive");
    if (in->n_levels <= 0 || in->n_levels > in->n_nodes) return fail(PML_ERR_INVALID, "n_levels must lie in [1, n_nodes]");
    if (!in->level_offsets || !in->parent || !in->dist || !in->given || !in->root_dates || !out->date)
        return fail(PML_ERR_INVALID, "NULL array");
    if (!in->dates_only) {
        if (in->n_configs <= 0 || in->n_tips <= 0 || in->n_vertices <= 0)
            return fail(PML_ERR_INVALID, "n_configs, n_tips and n_vertices must be positive");
        if (in->n_milestones <= 0) return fail(PML_ERR_INVALID, "n_milestones must be positive");
        if (in->n_milestones > 64) return fail(PML_ERR_UNSUPPORTED, "%d milestones; at most 64 are supported", in->n_milestones);
        if (in->timeline_type < 0 || in->timeline_type > 2) return fail(PML_ERR_INVALID, "timeline_type must be 0 (SAMPLED), 1 (NODES) or 2 (LTT)");
        if (!in->alive || !in->up || !in->config || !in->is_tip || !in->is_polytomy || !in->top || !in->below_lo || !in->below_hi ||
            !in->tip_order || !in->member_offsets || !in->milestones || !out->get_date || !out->n_roots || !out->tips_min ||
            !out->tips_max || !out->internal_min || !out->internal_max || !out->below_min || !out->below_max || !out->first_milestone)
            return fail(PML_ERR_INVALID, "NULL array");
    }
    return launch_timeline(ctx, *in, *out);
}

int pml_timeline_info(pml_ctx* ctx, double* stage_ms, int32_t* levels, int64_t* launches, int64_t* date_launches, int32_t* fuse_width) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (stage_ms)
        for (int i = 0; i < 6; ++i) stage_ms[i] = ctx->tl_ms[i];
    if (levels) *levels = ctx->tl_levels;
    if (launches) *launches = ctx->tl_launches;
    if (date_launches) *date_launches = ctx->tl_date_launches;
    if (fuse_width) *fuse_width = PML_TL_FUSE_WIDTH;
    return PML_OK;
}

int pml_select_states(pml_ctx* ctx, int method, int force_joint, const uint64_t* lh_mask, uint64_t* masks_out,
                      int32_t* n_states_out) {
    PML_TRY(require_model(ctx));
    if (!ctx->results.posteriors_exist()) return fail(PML_ERR_INVALID, "pml_select_states needs pml_top_down_marginals first");
    if (method != 0 && method != 1) return fail(PML_ERR_INVALID, "method must be 0 (MAP) or 1 (MPPA)");
    if (method == 1 && force_joint && !ctx->results.joint_states_exist())
        return fail(PML_ERR_INVALID, "force_joint needs the joint states of a pml_joint_backtrace");
    PML_TRY(materialize_tip_posteriors(ctx));  // the selection reads every row, and rewrites the masks
    note_tips_observed(ctx, 0, ctx->C, false);  // (masks from now on: whatever was selected)
    const size_t CN = (size_t)ctx->C * ctx->N;
    if (!ctx->d_nsel) PML_TRY(dev_alloc(ctx, &ctx->d_nsel, CN));
    if (lh_mask && ctx->k % 64) {
        const u64 valid = (1ull << (ctx->k % 64)) - 1ull;
        for (size_t i = ctx->W - 1; i < CN * ctx->W; i += ctx->W)
            if (lh_mask[i] & ~valid) return fail(PML_ERR_INVALID, "lh_mask word %zu has bits beyond k", i);
    }
    std::vector<u64> lh_mask_own;   // (the caller's rows in the library's numbering)
    CallScope mem(ctx->stream, false);
    u64* d_lh_mask = nullptr;
    if (lh_mask) {
        const u64* src = (const u64*)lh_mask;
        if (permuted(ctx)) {
            lh_mask_own.resize(CN * ctx->W);
            rows_to_internal(ctx, src, lh_mask_own.data(), (size_t)ctx->W, (size_t)ctx->C);
            src = lh_mask_own.data();
        }
        PML_TRY(mem.put(&d_lh_mask, src, CN * ctx->W));
    }
    ctx->results.tip_rows_unknown();   // (before the masks are rewritten)
    PML_TRY(dispatch_select(ctx, method, force_joint, d_lh_mask));   // pml_launch_matrix.hip
    HIP_TRY(hipGetLastError());
    PML_TRY(fetch_rows(ctx, (const u64*)ctx->d_masks, (size_t)ctx->W, (size_t)ctx->W, (size_t)ctx->C, (u64*)masks_out));
    PML_TRY(fetch_rows(ctx, ctx->d_nsel, 1, 1, (size_t)ctx->C, n_states_out));
    PML_TRY(mem.finish());
    // the columns' masks changed: sweeps must be redone, the posteriors themselves stay valid for inspection
    ctx->results.masks_selected();
    return PML_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
static int fetch_vectors(pml_ctx* ctx, const double* src, int col, double* out) {
    const size_t N = ctx->N;
    if (ctx->ks == ctx->k) {
        HIP_TRY(hipMemcpyAsync(out, src + (size_t)col * N * ctx->ks, N * ctx->k * sizeof(double), hipMemcpyDeviceToHost,
                               ctx->stream));
    } else {
        HIP_TRY(hipMemcpy2DAsync(out, ctx->k * sizeof(double), src + (size_t)col * N * ctx->ks, ctx->ks * sizeof(double),
                                 ctx->k * sizeof(double), N, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return PML_OK;
}

static int fetch_exponents(pml_ctx* ctx, const i64* src, int col, double* out) {
    std::vector<i64> tmp(ctx->N);
    HIP_TRY(hipMemcpyAsync(tmp.data(), src + (size_t)col * ctx->N, ctx->N * sizeof(i64), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const double l2 = std::log10(2.0);
    for (int i = 0; i < ctx->N; ++i) out[i] = -(double)tmp[i] * l2;
    return PML_OK;
}

// after a fused sweep the cherries' bottom-up vectors only ever existed in registers: compute them for inspection
PML_INTERNAL int materialize_cherries(pml_ctx* ctx) {
    if (ctx->results.children_missing()) {
        // the children of the two-level units: their own units (two cherries of two tips), from the tips
        PML_TRY(dispatch_sweep(ctx, SW_BU_MARG_FUSED_NOVEC, L_CHILD_UNITS, 0, ctx->sup.n_child_units));  // (nothing if 0)
        // ... and the children of the stacked units (two stored children each; in chunks of at most 65 536 units: the
        // lane shape, hence the rounding of pi . v, of the levels they were taken from)
        for (int a = 0; a < 2 * ctx->sup.n_stack; a += 65536)
            PML_TRY(dispatch_sweep(ctx, SW_BU_MARG_FUSED, L_STACK_CHILDREN, a, std::min(65536, 2 * ctx->sup.n_stack - a)));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->results.children_written();
    }
    if (!ctx->results.cherries_missing()) return PML_OK;
    PML_TRY(dispatch_sweep(ctx, ctx->results.cherries_joint() ? SW_BU_CHERRIES_JOINT : SW_BU_CHERRIES, L_CHERRIES, 0, ctx->n_cherries));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->results.cherries_written();
    return PML_OK;
}

static int need_top_down(pml_ctx* ctx) {
    return ctx->results.has_top_down() ? PML_OK : fail(PML_ERR_INVALID, "no valid top-down sweep");
}
static int need_joint_states(pml_ctx* ctx) {
    return ctx->results.has_joint_states() ? PML_OK : fail(PML_ERR_INVALID, "no valid joint back-trace");
}

static int download_internal(pml_ctx* ctx, int what, int32_t col, void* out);

int pml_download(pml_ctx* ctx, int what, int32_t col, void* out) {
    PML_TRY(download_internal(ctx, what, col, out));   // rows in the library's numbering
    if (permuted(ctx)) {
        switch (what) {
            case PML_BUF_BU:
            case PML_BUF_TD:
            case PML_BUF_POSTERIOR:
                rows_to_api_inplace(ctx, (double*)out, (size_t)ctx->k, 1);
                break;
            case PML_BUF_JOINT_TABLE:
                rows_to_api_inplace(ctx, (int32_t*)out, (size_t)ctx->k, 1);
                break;
            case PML_BUF_JOINT_STATE:
                rows_to_api_inplace(ctx, (int32_t*)out, 1, 1);
                break;
            default:
                rows_to_api_inplace(ctx, (double*)out, 1, 1);
                break;
        }
    }
    return PML_OK;
}

static int download_internal(pml_ctx* ctx, int what, int32_t col, void* out) {
    PML_TRY(require_model(ctx));
    if (col < 0 || col >= ctx->C || !out) return fail(PML_ERR_INVALID, "bad column / output");
    // (a pass that ended in a spin on the completion word may have left the stream busy, and the blocking copies below run
    // on the NULL stream, which a non-blocking stream is not ordered with)
    PML_TRY(wait_pending(ctx, true));
    if (what == PML_BUF_BU || what == PML_BUF_BU_SF) PML_TRY(materialize_cherries(ctx));
    const size_t N = ctx->N;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    switch (what) {
        case PML_BUF_BU: {
            if (!ctx->results.has_bottom_up()) return fail(PML_ERR_INVALID, "no valid bottom-up sweep");
            double* o = (double*)out;
            PML_TRY(fetch_vectors(ctx, ctx->d_bu, col, o));
            std::vector<u64> m(N * ctx->W);
            HIP_TRY(hipMemcpy(m.data(), ctx->d_masks + (size_t)col * N * ctx->W, m.size() * sizeof(u64), hipMemcpyDeviceToHost));
            for (size_t n = 0; n < N; ++n)
                if (ctx->forest.n_children[n] == 0)
                    for (int s = 0; s < ctx->k; ++s) o[n * ctx->k + s] = (double)((m[n * ctx->W + (s >> 6)] >> (s & 63)) & 1ull);
            return PML_OK;
        }
        case PML_BUF_BU_SF: {
            if (!ctx->results.has_bottom_up()) return fail(PML_ERR_INVALID, "no valid bottom-up sweep");
            PML_TRY(fetch_exponents(ctx, ctx->d_be, col, (double*)out));
            for (size_t n = 0; n < N; ++n)
                if (ctx->forest.n_children[n] == 0) ((double*)out)[n] = 0.0;
            return PML_OK;
        }
        case PML_BUF_TD:
            PML_TRY(need_top_down(ctx));
            PML_TRY(materialize_td(ctx));
            return fetch_vectors(ctx, ctx->d_td, col, (double*)out);
        case PML_BUF_TD_SF:
            PML_TRY(need_top_down(ctx));
            PML_TRY(materialize_td(ctx));
            return fetch_exponents(ctx, ctx->d_te, col, (double*)out);
        case PML_BUF_POSTERIOR:
            PML_TRY(need_top_down(ctx));
            PML_TRY(materialize_tip_posteriors(ctx));
            return fetch_vectors(ctx, ctx->d_post, col, (double*)out);
        case PML_BUF_LH_SUM:
            PML_TRY(need_top_down(ctx));
            HIP_TRY(hipMemcpy(out, ctx->d_lhsum + (size_t)col * N, N * sizeof(double), hipMemcpyDeviceToHost));
            return PML_OK;
        case PML_BUF_LH_SF:
            PML_TRY(need_top_down(ctx));
            return fetch_exponents(ctx, ctx->d_lhe, col, (double*)out);
        case PML_BUF_JOINT_TABLE: {
            if (!ctx->results.has_joint()) return fail(PML_ERR_INVALID, "no valid joint sweep");
            // the tables hold one byte per entry on the device (two beyond 256 states); the interface hands out int32
            const size_t width = ctx->k > 256 ? 2 : 1;
            std::vector<pml_jt> tmp(N * ctx->ks * width);
            HIP_TRY(hipMemcpy(tmp.data(), ctx->d_J + (size_t)col * N * ctx->ks * width, tmp.size(), hipMemcpyDeviceToHost));
            int32_t* o = (int32_t*)out;
            const unsigned short* wide = reinterpret_cast<const unsigned short*>(tmp.data());
            for (size_t n = 0; n < N; ++n)
                for (int i = 0; i < ctx->k; ++i) o[n * ctx->k + i] = width == 2 ? (int32_t)wide[n * ctx->ks + i] : (int32_t)tmp[n * ctx->ks + i];
            return PML_OK;
        }
        case PML_BUF_JOINT_STATE:
            PML_TRY(need_joint_states(ctx));
            HIP_TRY(hipMemcpy(out, ctx->d_js + (size_t)col * N, N * sizeof(int), hipMemcpyDeviceToHost));
            return PML_OK;
        case PML_BUF_BRANCH_EXP:
            if (ctx->kind != PML_MODEL_F81) return fail(PML_ERR_INVALID, "branch exponentials exist for the F81 family only");
            PML_TRY(run_prep(ctx));
            HIP_TRY(hipStreamSynchronize(ctx->stream));
            HIP_TRY(hipMemcpy(out, ctx->d_E + (size_t)col * N, N * sizeof(double), hipMemcpyDeviceToHost));
            return PML_OK;
        default:
            return fail(PML_ERR_INVALID, "unknown buffer id %d", what);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// multi-GPU: one collective, the sum of the per-rank log-likelihoods
int pml_comm_unique_id(unsigned char* id_out) {
    if (!id_out) return fail(PML_ERR_INVALID, "id_out is NULL");
    PmlRccl* r = pml_rccl();
    if (!r->handle) return fail(PML_ERR_UNSUPPORTED, "librccl could not be loaded: %s", r->error.c_str());
    ncclUniqueId id;
    const ncclResult_t e = r->GetUniqueId(&id);
    if (e != ncclSuccess) return fail(PML_ERR_HIP, "ncclGetUniqueId failed: %s", r->GetErrorString(e));
    static_assert(sizeof(id.internal) == PML_COMM_ID_BYTES, "unique id size");
    memcpy(id_out, id.internal, PML_COMM_ID_BYTES);
    return PML_OK;
}

int pml_comm_init(pml_ctx* ctx, int rank, int world, const unsigned char* id) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    if (world < 1 || rank < 0 || rank >= world) return fail(PML_ERR_INVALID, "rank %d out of 0..%d", rank, world - 1);
    if (ctx->comm) return fail(PML_ERR_INVALID, "the ctx already has a communicator");
    HIP_TRY(hipSetDevice(ctx->device));
    PmlComm* c = new PmlComm();
    c->rank = rank;
    c->world = world;
    // PASTML_HIP_COMM_FORCE_RCCL: a world of one still goes through librccl (exercises the whole path on one GPU)
    if (world > 1 || getenv("PASTML_HIP_COMM_FORCE_RCCL")) {
        if (!id) {
            delete c;
            return fail(PML_ERR_INVALID, "id is NULL");
        }
        PmlRccl* r = pml_rccl();
        if (!r->handle) {
            delete c;
            return fail(PML_ERR_UNSUPPORTED, "librccl could not be loaded: %s", r->error.c_str());
        }
        ncclUniqueId uid;
        memcpy(uid.internal, id, PML_COMM_ID_BYTES);
        const ncclResult_t e = r->CommInitRank(&c->comm, world, uid, rank);
        if (e != ncclSuccess) {
            delete c;
            return fail(PML_ERR_HIP, "ncclCommInitRank failed: %s", r->GetErrorString(e));
        }
    }
    if (hipMalloc((void**)&c->d_total, sizeof(double)) != hipSuccess ||
        hipHostMalloc((void**)&c->h_total, sizeof(double)) != hipSuccess) {
        if (c->comm) (void)pml_rccl()->CommDestroy(c->comm);
        if (c->d_total) (void)hipFree(c->d_total);
        delete c;
        return fail(PML_ERR_HIP, "allocation of the communicator's buffers failed");
    }
    ctx->comm = c;
    return PML_OK;
}

int pml_comm_info(pml_ctx* ctx, int32_t* rank, int32_t* world, int32_t* backend, int32_t* rccl_ranks) {
    if (!ctx || !ctx->comm) return fail(PML_ERR_INVALID, "no communicator: call pml_comm_init first");
    const PmlComm* c = ctx->comm;
    if (rank) *rank = c->rank;
    if (world) *world = c->world;
    if (backend) *backend = c->comm ? 1 : 0;
    if (rccl_ranks) {
        *rccl_ranks = 0;
        if (c->comm) {
            PmlRccl* r = pml_rccl();
            int n = -1;
            if (r->CommCount) {
                const ncclResult_t e = r->CommCount(c->comm, &n);
                if (e != ncclSuccess) return fail(PML_ERR_HIP, "ncclCommCount failed: %s", r->GetErrorString(e));
            }
            *rccl_ranks = n;
        }
    }
    return PML_OK;
}

int pml_device_uuid(int device, char* uuid_out) {
    if (!uuid_out) return fail(PML_ERR_INVALID, "uuid_out is NULL");
    hipUUID id;
    HIP_TRY(hipDeviceGetUuid(&id, device));
    static const char hex[] = "0123456789abcdef";
    for (int i = 0; i < 16; ++i) {
        const unsigned char b = (unsigned char)id.bytes[i];
        uuid_out[2 * i] = hex[b >> 4];
        uuid_out[2 * i + 1] = hex[b & 15];
    }
    uuid_out[32] = 0;
    return PML_OK;
}

int pml_comm_destroy(pml_ctx* ctx) {
    if (!ctx || !ctx->comm) return PML_OK;
    PmlComm* c = ctx->comm;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (c->comm) (void)pml_rccl()->CommDestroy(c->comm);
    if (c->d_buf) (void)hipFree(c->d_buf);
    if (c->h_buf) (void)hipHostFree(c->h_buf);
    if (c->d_total) (void)hipFree(c->d_total);
    if (c->h_total) (void)hipHostFree(c->h_total);
    delete c;
    ctx->comm = nullptr;
    return PML_OK;
}

int pml_comm_allreduce(pml_ctx* ctx, const double* in, double* out, int32_t count, int op) {
    if (!ctx || !ctx->comm) return fail(PML_ERR_INVALID, "no communicator: call pml_comm_init first");
    if (!in || !out || count <= 0) return fail(PML_ERR_INVALID, "bad in / out / count");
    if (op != PML_COMM_SUM && op != PML_COMM_MAX) return fail(PML_ERR_INVALID, "op must be PML_COMM_SUM or PML_COMM_MAX");
    PmlComm* c = ctx->comm;
    if (!c->comm) {
        if (out != in) memmove(out, in, sizeof(double) * count);
        return PML_OK;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    if (c->cap < (size_t)count) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (c->d_buf) (void)hipFree(c->d_buf);
        if (c->h_buf) (void)hipHostFree(c->h_buf);
        c->d_buf = c->h_buf = nullptr;
        c->cap = 0;
        const size_t cap = std::max<size_t>(64, (size_t)count);
        HIP_TRY(hipMalloc((void**)&c->d_buf, cap * sizeof(double)));
        HIP_TRY(hipHostMalloc((void**)&c->h_buf, cap * sizeof(double)));
        c->cap = cap;
    }
    memcpy(c->h_buf, in, sizeof(double) * count);
    HIP_TRY(hipMemcpyAsync(c->d_buf, c->h_buf, sizeof(double) * count, hipMemcpyHostToDevice, ctx->stream));
    PmlRccl* r = pml_rccl();
    const ncclResult_t e = r->AllReduce(c->d_buf, c->d_buf, (size_t)count, ncclDouble, op == PML_COMM_SUM ? ncclSum : ncclMax,
                                        c->comm, ctx->stream);
    if (e != ncclSuccess) return fail(PML_ERR_HIP, "ncclAllReduce failed: %s", r->GetErrorString(e));
    HIP_TRY(hipMemcpyAsync(c->h_buf, c->d_buf, sizeof(double) * count, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, c->h_buf, sizeof(double) * count);
    return PML_OK;
}

int pml_allreduce_loglik(pml_ctx* ctx, const double* loglik, int32_t n_cols, double* total_out) {
    if (!loglik || !total_out || n_cols <= 0) return fail(PML_ERR_INVALID, "bad loglik / total_out / n_cols");
    // the local sum in column order (as pastml/acr.py would add the characters' results up), then one 8-byte all-reduce
    double local = 0.0;
    for (int i = 0; i < n_cols; ++i) local += loglik[i];
    return pml_comm_allreduce(ctx, &local, total_out, 1, PML_COMM_SUM);
}

int pml_loglik_total(pml_ctx* ctx, double* total_out) {
    if (!ctx || !ctx->comm) return fail(PML_ERR_INVALID, "no communicator: call pml_comm_init first");
    if (!total_out) return fail(PML_ERR_INVALID, "total_out is NULL");
    if (!ctx->comm->total_fresh) return fail(PML_ERR_INVALID, "no pml_marginal_pass since the last pml_loglik_total");
    *total_out = ctx->comm->h_total[0];  // (pml_marginal_pass has waited for the stream)
    ctx->comm->total_fresh = false;
    return PML_OK;
}

// numpy's pairwise summation of a contiguous run (numpy/_core/src/umath/loops_utils.h.src, pairwise_sum: what
// ndarray.sum() does along a contiguous axis): the frequencies must come out with numpy's bits, because the decoded
// points are what the reference-side arithmetic (models/__init__.py:328-330) would hand to the sweeps
static double np_pairwise_sum(const double* a, int n) {
    if (n < 8) {
        double res = 0.0;
        for (int i = 0; i < n; ++i) res += a[i];
        return res;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

int pml_host_f81_fd_points(int32_t n, int32_t k, const double* x, const double* lower, const double* upper, int32_t opt_sf,
                           int32_t opt_tau, int32_t free_pi, double sf_fixed, double tau_fixed, const double* pi_fixed,
                           double forest_length, double num_nodes, double* pi_out, double* sf_out, double* tau_out,
                           double* tf_out, double* steps_out, double step) {
    if (n < 0 || k < 1 || !x || !lower || !upper || !pi_out || !sf_out || !tau_out || !tf_out || (n > 0 && !steps_out))
        return fail(PML_ERR_INVALID, "NULL array / bad sizes");
    if (n != (opt_sf ? 1 : 0) + (opt_tau ? 1 : 0) + (free_pi ? k - 1 : 0))
        return fail(PML_ERR_INVALID, "n = %d does not match the parameter layout", n);
    if (!free_pi && !pi_fixed) return fail(PML_ERR_INVALID, "pi_fixed is NULL");
    if (!(step > 0.0)) return fail(PML_ERR_INVALID, "step must be positive");
    const double h = step;
    for (int i = 0; i < n; ++i) {
        const volatile double moved = x[i] + h;   // (scipy: the step as the floating-point numbers see it)
        const double step = moved - x[i];
        if (step == 0.0 || moved < lower[i] || moved > upper[i] || !(x[i] >= lower[i] && x[i] <= upper[i]))
            return PML_ERR_UNSUPPORTED;
    }
    std::vector<double> ratios((size_t)k);
    for (int row = 0; row <= n; ++row) {
        const int moved = row - 1;   // row 0 is x itself
        auto at = [&](int i) { return i == moved ? x[i] + h : x[i]; };
        int pos = 0;
        const double sf = opt_sf ? at(pos++) : sf_fixed;
        const double tau = opt_tau ? at(pos++) : tau_fixed;
        sf_out[row] = sf;
        tau_out[row] = tau;
        tf_out[row] = tau != 0.0 ? forest_length / (forest_length + tau * (num_nodes - 1.0)) : 1.0;
        double* pi = pi_out + (size_t)row * k;
        if (free_pi) {
            for (int j = 0; j < k - 1; ++j) ratios[j] = at(pos + j);
            ratios[k - 1] = 1.0;
            const double total = np_pairwise_sum(ratios.data(), k);
            for (int j = 0; j < k; ++j) pi[j] = ratios[j] / total;
        } else {
            memcpy(pi, pi_fixed, sizeof(double) * k);
        }
        if (moved >= 0) steps_out[moved] = (x[moved] + h) - x[moved];
    }
    return PML_OK;
}

int pml_device_sync(int device) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipDeviceSynchronize());
    return PML_OK;
}

int pml_download_strided(pml_ctx* ctx, int what, int32_t col, int32_t first, int32_t stride, int32_t count, void* out) {
    PML_TRY(require_model(ctx));
    if (col < 0 || col >= ctx->C || !out) return fail(PML_ERR_INVALID, "bad column / output");
    if (first < 0 || stride < 1 || count < 1 || (long long)first + (long long)(count - 1) * stride >= ctx->N)
        return fail(PML_ERR_INVALID, "rows first=%d stride=%d count=%d leave 0..%d", first, stride, count, ctx->N - 1);
    const size_t N = ctx->N;
    const void* src = nullptr;
    size_t row_bytes = 0, src_row_bytes = 0;
    switch (what) {
        case PML_BUF_POSTERIOR:
            PML_TRY(need_top_down(ctx));
            PML_TRY(materialize_tip_posteriors(ctx));
            src = ctx->d_post + ((size_t)col * N + first) * ctx->ks;
            row_bytes = ctx->k * sizeof(double);
            src_row_bytes = ctx->ks * sizeof(double);
            break;
        case PML_BUF_LH_SUM:
            PML_TRY(need_top_down(ctx));
            src = ctx->d_lhsum + (size_t)col * N + first;
            row_bytes = src_row_bytes = sizeof(double);
            break;
        case PML_BUF_LH_SF:
            PML_TRY(need_top_down(ctx));
            src = ctx->d_lhe + (size_t)col * N + first;
            row_bytes = src_row_bytes = sizeof(i64);
            break;
        case PML_BUF_JOINT_STATE:
            PML_TRY(need_joint_states(ctx));
            src = ctx->d_js + (size_t)col * N + first;
            row_bytes = src_row_bytes = sizeof(int);
            break;
        default:
            return fail(PML_ERR_INVALID, "pml_download_strided serves PML_BUF_POSTERIOR, _LH_SUM, _LH_SF, _JOINT_STATE");
    }
    if (permuted(ctx)) {
        // the rows asked for are scattered in the library's numbering: gathered on the device, copied once (round 5 issued one
        // small copy per row, ~10 us each)
        const char* col0 = (const char*)src - (size_t)first * src_row_bytes;   // (src points at row `first`: back to the column's row 0)
        const size_t bytes = (size_t)count * row_bytes;
        if (ctx->stage_bytes < bytes) {
            if (ctx->d_stage) (void)hipFree(ctx->d_stage);
            ctx->d_stage = nullptr;
            ctx->stage_bytes = 0;
            HIP_TRY(hipMalloc(&ctx->d_stage, bytes));
            ctx->stage_bytes = bytes;
        }
        const int wd = (int)(row_bytes / 4), ws = (int)(src_row_bytes / 4);
        const long long total = (long long)count * wd;
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)std::min<long long>((total + PML_BLOCK - 1) / PML_BLOCK, 65536)),
                           dim3(PML_BLOCK), 0, ctx->stream, (const unsigned*)col0, (unsigned*)ctx->d_stage, ctx->d_new_of_old,
                           (long long)count, wd, ws, first, stride);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, ctx->d_stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        HIP_TRY(hipMemcpy2DAsync(out, row_bytes, src, src_row_bytes * stride, row_bytes, count, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (what == PML_BUF_LH_SF) {  // base-2 exponents -> the reference's base-10 scale, in place (same width)
        const double l2 = std::log10(2.0);
        i64* e = (i64*)out;
        double* o = (double*)out;
        for (int i = 0; i < count; ++i) o[i] = -(double)e[i] * l2;
    }
    return PML_OK;
}

int pml_profile_enable(pml_ctx* ctx, int on) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    ctx->profile = on != 0;
    return PML_OK;
}

int pml_profile_read(pml_ctx* ctx, int which, double* total_ms, int64_t* launches, int reset) {
    if (!ctx || which < 0 || which > 4) return fail(PML_ERR_INVALID, "bad profile slot");
    PML_TRY(prof_drain(ctx));
    if (total_ms) *total_ms = ctx->prof_ms[which];
    if (launches) *launches = ctx->prof_launches[which];
    if (reset) {
        ctx->prof_ms[which] = 0;
        ctx->prof_launches[which] = 0;
    }
    return PML_OK;
}

int pml_timer_start(pml_ctx* ctx) {
    if (!ctx) return fail(PML_ERR_INVALID, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
    return PML_OK;
}

int pml_timer_stop(pml_ctx* ctx, float* milliseconds) {
    if (!ctx || !milliseconds) return fail(PML_ERR_INVALID, "NULL argument");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(hipEventSynchronize(ctx->ev1));
    HIP_TRY(hipEventElapsedTime(milliseconds, ctx->ev0, ctx->ev1));
    return PML_OK;
}

