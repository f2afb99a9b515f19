// Host-only check of the windowed sweep plans (pastml_amd/csrc/pml_pij_window.h): plans forests with pml_schedule.cpp, takes the
// plans of the sweeps that read P(t) (BU_PLAIN, TD_LEVELS) and cuts them with pml_plan_pij_window for windows of the largest
// fan-out, of three more, and of the whole forest.  Checked: every non-root branch is built exactly once per sweep, in the run
// that reads it; slots inside a run are distinct and below B; no parent is split; runs keep the level order; the concatenated
// sweep records cover the plan's records exactly; the signal record is last; a window below the fan-out is refused.
// Built and run by tests/test_pij_window_plan_host.py; prints FAIL lines and exits 1, or one OK line.
#include "../pastml_amd/csrc/pml_pij_window.h"

#include <algorithm>
#include <cstdio>
#include <functional>
#include <random>

static int g_failures = 0;
static std::string g_case;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++g_failures <= 40) {                     \
                printf("FAIL [%s] ", g_case.c_str());     \
                printf(__VA_ARGS__);                      \
                printf("\n");                             \
            }                                             \
        }                                                 \
    } while (0)

// ---- forests: ids in breadth-first order, a node's children next to each other (what pml_tree_upload is given)
struct Tree {
    int n_roots = 0;
    std::vector<int> parent, first_child, n_children, post_rank, bu_offsets, bu_order, td_offsets, td_parent_offsets, td_parents;
    std::vector<double> dist;
};
// budgets: tips below each root; split(tips of a node) -> tips of its children
static Tree grow(const std::vector<int>& budgets, const std::function<std::vector<int>(int)>& split) {
    Tree T;
    T.n_roots = (int)budgets.size();
    std::vector<int> budget = budgets, depth(budgets.size(), 0);
    T.parent.assign(budgets.size(), -1);
    for (size_t i = 0; i < budget.size(); ++i) {
        T.first_child.push_back(0);
        T.n_children.push_back(0);
        if (budget[i] <= 1) continue;
        const std::vector<int> parts = split(budget[i]);
        T.first_child[i] = (int)budget.size();
        T.n_children[i] = (int)parts.size();
        for (int b : parts) {
            budget.push_back(b);
            depth.push_back(depth[i] + 1);
            T.parent.push_back((int)i);
        }
    }
    const int N = (int)budget.size();
    T.dist.assign(N, 1.0);
    T.post_rank.resize(N);
    std::vector<int> height(N, 0);
    int max_h = 0, max_d = 0;
    for (int i = N - 1; i >= 0; --i) {
        T.post_rank[i] = i;
        for (int j = 0; j < T.n_children[i]; ++j) height[i] = std::max(height[i], 1 + height[T.first_child[i] + j]);
        max_h = std::max(max_h, height[i]);
        max_d = std::max(max_d, depth[i]);
    }
    T.bu_offsets.assign(1, 0);
    for (int h = 1; h <= max_h; ++h) {
        for (int i = 0; i < N; ++i)
            if (height[i] == h) T.bu_order.push_back(i);
        T.bu_offsets.push_back((int)T.bu_order.size());
    }
    T.td_offsets.assign(1, 0);
    T.td_parent_offsets.assign(1, 0);
    for (int d = 0, i = 0; d <= max_d; ++d) {
        for (; i < N && depth[i] == d; ++i)
            if (T.n_children[i] > 0) T.td_parents.push_back(i);
        T.td_offsets.push_back(i);
        T.td_parent_offsets.push_back((int)T.td_parents.size());
    }
    return T;
}

static std::mt19937 g_rng(4711);
static std::vector<int> split_even(int n) { return {n - n / 2, n / 2}; }
static std::vector<int> split_comb(int n) { return {n - 1, 1}; }
static std::vector<int> split_star(int n) { return std::vector<int>((size_t)n, 1); }
static std::vector<int> split_ragged(int n) {   // a quarter of the nodes are polytomies of three to seven children
    const int want = (g_rng() % 100 < 25) ? 3 + (int)(g_rng() % 5) : 2;
    std::vector<int> parts((size_t)std::min(want, n), 1);
    for (int left = n - (int)parts.size(); left > 0; --left) ++parts[g_rng() % parts.size()];
    return parts;
}

// the window of one sweep: its plan of plain level launches, cut for B branches
static void check_sweep(const PmlForest& f, const std::vector<int>& bu_order, const std::vector<int>& td_parents,
                        const std::vector<PmlLaunch>& plan, bool bottom_up, long long B) {
    PmlWindowPlan W;
    const std::string bad = pml_plan_pij_window(plan, f, bu_order, td_parents, B, W);
    CHECK(bad.empty(), "refused: %s", bad.c_str());
    if (!bad.empty()) return;
    const std::vector<int>& nodes = bottom_up ? bu_order : td_parents;
    const int want_list = bottom_up ? L_BU_PLAIN : L_TD_PLAIN;
    // (1) the sweep records, concatenated, are the plan's records: a cut record's pieces are consecutive ranges that add up to it
    size_t s = 0;
    for (size_t i = 0; i < plan.size(); ++i) {
        const PmlLaunch& r = plan[i];
        const bool level = r.op == OP_LEVEL && r.list == want_list && r.count > 0;
        CHECK(s < W.steps.size(), "the windowed sequence ends before record %zu", i);
        if (s >= W.steps.size()) return;
        if (!level) {
            const PmlWindowStep& w = W.steps[s++];
            CHECK(w.build_count == 0, "record %zu (op %d) builds %d branches", i, r.op, w.build_count);
            CHECK(w.launch.op == r.op && w.launch.list == r.list && w.launch.kind == r.kind && w.launch.first == r.first &&
                      w.launch.count == r.count && w.launch.signal == r.signal && w.launch.bracket == r.bracket &&
                      w.launch.arg == r.arg && w.launch.branch == r.branch && w.launch.cherries == r.cherries,
                  "record %zu (op %d) changed", i, r.op);
            continue;
        }
        int at = r.first;
        while (at < r.first + r.count) {
            CHECK(s < W.steps.size(), "level record %zu is not covered beyond entry %d", i, at);
            if (s >= W.steps.size()) return;
            const PmlWindowStep& w = W.steps[s++];
            CHECK(w.launch.op == OP_LEVEL && w.launch.list == r.list && w.launch.kind == r.kind && w.launch.bracket == r.bracket &&
                      w.launch.branch == r.branch,
                  "a run of record %zu is another kind of launch", i);
            CHECK(w.launch.first == at && w.launch.count > 0, "a run of record %zu starts at %d, not %d (count %d)", i, w.launch.first, at,
                  w.launch.count);
            if (w.launch.count <= 0) return;
            at += w.launch.count;
            // (a run never crosses a level boundary: it lies inside its record, which is one level)
            CHECK(at <= r.first + r.count, "a run of record %zu crosses the end of its level", i);
            CHECK(w.launch.signal == (r.signal && at == r.first + r.count), "signal flag of a run of record %zu", i);
        }
    }
    CHECK(s == W.steps.size(), "%zu records beyond the plan", W.steps.size() - s);
    // (2) per run: it builds exactly the children of its parents (no parent split), in slots 0 .. below B, and nothing else
    std::vector<int> built((size_t)f.N, 0);
    int build_at = 0, runs = 0;
    for (const PmlWindowStep& w : W.steps) {
        CHECK(w.build_count >= 0 && w.build_count <= B, "a run of %d branches for a window of %lld", w.build_count, B);
        if (w.build_count == 0) continue;
        ++runs;
        CHECK(w.build_first == build_at, "run builds from %d, the list is at %d", w.build_first, build_at);
        CHECK((size_t)w.build_first + (size_t)w.build_count <= W.branches.size(), "run beyond the branch list");
        if ((size_t)w.build_first + (size_t)w.build_count > W.branches.size()) return;
        build_at = w.build_first + w.build_count;
        std::vector<int> want, slots;
        for (int q = w.launch.first; q < w.launch.first + w.launch.count; ++q)
            for (int j = 0; j < f.n_children[nodes[q]]; ++j) want.push_back(f.first_child[nodes[q]] + j);
        std::vector<int> got(W.branches.begin() + w.build_first, W.branches.begin() + w.build_first + w.build_count);
        CHECK(got == want, "a run over %d parents builds %zu branches, its parents have %zu children", w.launch.count, got.size(),
              want.size());
        for (int i = 0; i < w.build_count; ++i) {
            const int ch = W.branches[w.build_first + i];
            ++built[ch];
            CHECK(W.slot[ch] == i, "branch %d is built into slot %d and looked up in slot %d", ch, i, W.slot[ch]);
            slots.push_back(W.slot[ch]);
        }
        std::sort(slots.begin(), slots.end());
        CHECK(std::adjacent_find(slots.begin(), slots.end()) == slots.end(), "two branches of a run share a slot");
        CHECK(slots.empty() || (slots.front() >= 0 && slots.back() < B), "slot beyond the window");
    }
    CHECK(build_at == (int)W.branches.size(), "%zu branches are listed and never built", W.branches.size() - (size_t)build_at);
    CHECK(runs == W.runs, "%d runs build something, the plan says %d", runs, W.runs);
    // (3) every non-root branch exactly once per sweep, the roots never
    for (int n = 0; n < f.N; ++n) {
        CHECK(built[n] == (f.parent[n] >= 0 ? 1 : 0), "branch %d (parent %d) is built %d times", n, f.parent[n], built[n]);
        if (f.parent[n] < 0) CHECK(W.slot[n] == -1, "root %d has slot %d", n, W.slot[n]);
    }
    // (4) the signal record, if any, is last; a whole-forest window cuts nothing
    for (size_t i = 0; i + 1 < W.steps.size(); ++i) CHECK(!W.steps[i].launch.signal, "record %zu of %zu signals", i, W.steps.size());
    if (B >= f.N) CHECK(W.steps.size() == plan.size(), "a window of the whole forest cut %zu records into %zu", plan.size(), W.steps.size());
}

static void run_forest(const char* name, const Tree& T) {
    PmlTreeArrays t = {(int)T.parent.size(), T.n_roots, (int)T.bu_offsets.size() - 1, (int)T.td_offsets.size() - 1,
                       T.parent.data(), T.first_child.data(), T.n_children.data(), T.bu_offsets.data(), T.bu_order.data(),
                       T.td_offsets.data(), T.td_parent_offsets.data(), T.td_parents.data(), T.post_rank.data(), T.dist.data()};
    g_case = name;
    const std::string bad = pml_check_tree(t);
    CHECK(bad.empty(), "bad forest: %s", bad.c_str());
    if (!bad.empty()) return;
    PmlTune tune;
    PmlNumbering num;
    PmlForest f = pml_plan_forest(t, tune, true, num);
    PmlTreePlan P = pml_plan_tree(f, t, tune);
    PmlThinPlan H = pml_plan_thin_ends(f, tune, 4096);
    const PmlSchedules S = {&P.blocks.s, &H.thin, &H.deep, &P.sup.s, &P.eig.s, &P.bt.s, &P.bu_level_vec_f, &P.bu_level_vec, &P.td_cherry_prefix};
    int n_internal = 0;
    for (int n = 0; n < f.N; ++n) n_internal += f.n_children[n] > 0;
    const std::vector<int> bu_order(t.bu_order, t.bu_order + n_internal), td_parents(t.td_parents, t.td_parents + n_internal);
    // an eigen model beyond 128 states with every fused sweep off: the sweeps that read P(t)
    PmlSweepTraits tr = {};
    tr.k = 130; tr.W = 3; tr.Gf = tr.Gt = 64;
    tr.fuse = true;
    tr.n_roots = T.n_roots;
    tr.n_cherries = (int)P.cherries.size();
    tr.waves = 4;
    tr.eig_nb = 1;
    const int fan = pml_window_max_fanout(f);
    int want_fan = 0;
    for (int n = 0; n < f.N; ++n) want_fan = std::max(want_fan, f.n_children[n]);
    CHECK(fan == want_fan, "largest fan-out %d, counted %d", fan, want_fan);
    char what[256];
    for (int C : {1, 3}) {
        tr.C = tr.sched_cols = C;
        const std::vector<PmlLaunch> plans[3] = {pml_plan_bottom_up(f, S, tr, true), pml_plan_bottom_up(f, S, tr, false),
                                                 pml_plan_top_down(f, S, tr, false)};
        CHECK(plans[0].front().branch == BU_PLAIN && plans[1].front().branch == BU_PLAIN && plans[2].front().branch == TD_LEVELS,
              "the plans are not the plain level sweeps");
        for (long long B : {(long long)fan, (long long)fan + 3, (long long)f.N, (long long)f.N + 1000}) {
            for (int p = 0; p < 3; ++p) {
                snprintf(what, sizeof(what), "%s C=%d B=%lld %s", name, C, B, p == 0 ? "bottom-up marginal" : p == 1 ? "bottom-up joint" : "top-down");
                g_case = what;
                check_sweep(f, bu_order, td_parents, plans[p], p < 2, B);
            }
        }
        // the two bottom-up sweeps walk the same level list: the same branch lists (one upload serves both)
        PmlWindowPlan a, b;
        (void)pml_plan_pij_window(plans[0], f, bu_order, td_parents, fan, a);
        (void)pml_plan_pij_window(plans[1], f, bu_order, td_parents, fan, b);
        CHECK(a.branches == b.branches && a.slot == b.slot, "the marginal and the joint sweep list different branches");
        // a plan whose last record signals keeps it last, on the last run only
        std::vector<PmlLaunch> sig = plans[2];
        sig.back().signal = true;
        snprintf(what, sizeof(what), "%s C=%d signalling top-down", name, C);
        g_case = what;
        check_sweep(f, bu_order, td_parents, sig, false, fan);
        // below the fan-out: refused, and the reason names the fan-out
        PmlWindowPlan none;
        g_case = std::string(name) + " refusal";
        const std::string why = pml_plan_pij_window(plans[0], f, bu_order, td_parents, fan - 1, none);
        CHECK(!why.empty() && why.find(std::to_string(fan)) != std::string::npos, "B = %d accepted or unexplained: '%s'", fan - 1, why.c_str());
        CHECK(none.steps.empty() && none.branches.empty(), "a refused window left a plan behind");
    }
}

int main() {
    run_forest("balanced", grow({256}, split_even));
    run_forest("caterpillar", grow({120}, split_comb));
    run_forest("star", grow({40}, split_star));
    run_forest("ragged", grow({700}, split_ragged));
    run_forest("forest", grow({300, 1}, split_ragged));
    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
