// Host-only check of the runs in which the consumers of P(t) outside the sweeps read it from the window
// (pastml_amd/csrc/pml_pij_window.h): the pieces of the exact counts (pml_window_piece_runs), the levels and frontier subtrees
// of the simulator and the scenario sampler (pml_plan_sim_window) and the level runs of the sampled counts (the top-down
// PmlWindowPlan), on a balanced tree, a 300-deep caterpillar, a star of 40 and a ragged forest with a single-tip tree, for
// windows of the largest fan-out, of 200 and of all nodes, and frontier depths 0, 3, 16 and the number of levels.
// Checked: every non-root branch a consumer reads is built exactly once per call, in the run that reads it; slots within a run
// are distinct and below B; the piece runs are whole pieces, in order, covering all ids; no frontier subtree is split; a subtree
// larger than B moves the frontier, never overflows; the launch count is at most levels + ceil(N / B) + the frontier's groups.
// Built and run by tests/test_pij_window_runs_host.py; prints FAIL lines and exits 1, or one OK line.
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

static std::mt19937 g_rng(4712);
static std::vector<int> split_even(int n) { return {n - n / 2, n / 2}; }
static std::vector<int> split_comb(int n) { return {n - 1, 1}; }
static std::vector<int> split_star(int n) { return std::vector<int>((size_t)n, 1); }
static std::vector<int> split_ragged(int n) {   // a quarter of the nodes are polytomies of three to seven children
    const int want = (g_rng() % 100 < 25) ? 3 + (int)(g_rng() % 5) : 2;
    std::vector<int> parts((size_t)std::min(want, n), 1);
    for (int left = n - (int)parts.size(); left > 0; --left) ++parts[g_rng() % parts.size()];
    return parts;
}

// the exact counts: ids in pieces of `piece`, a run is whole consecutive pieces whose ids fit B
static void check_pieces(int N, int piece, long long B) {
    std::vector<PmlPieceRun> runs;
    const std::string bad = pml_window_piece_runs(N, piece, B, runs);
    if (B < piece) {
        CHECK(!bad.empty() && runs.empty(), "a window of %lld below a piece of %d was accepted", B, piece);
        return;
    }
    CHECK(bad.empty(), "refused: %s", bad.c_str());
    const int n_pieces = (N + piece - 1) / piece;
    int at = 0;
    std::vector<int> built((size_t)N, 0);
    for (const PmlPieceRun& r : runs) {
        CHECK(r.p0 == at && r.p1 > r.p0 && r.p1 <= n_pieces, "run [%d, %d) after piece %d of %d", r.p0, r.p1, at, n_pieces);
        at = r.p1;
        const int i0 = r.p0 * piece, i1 = std::min(N, r.p1 * piece);
        CHECK(i1 - i0 <= B, "a run of %d ids for a window of %lld", i1 - i0, B);
        for (int i = i0; i < i1; ++i) {
            ++built[(size_t)i];
            CHECK(i - i0 >= 0 && i - i0 < B, "id %d in slot %d", i, i - i0);
        }
    }
    CHECK(at == n_pieces, "the runs end at piece %d of %d", at, n_pieces);
    for (int i = 0; i < N; ++i) CHECK(built[(size_t)i] == 1, "id %d is built %d times", i, built[(size_t)i]);
    CHECK((long long)runs.size() == (n_pieces + B / piece - 1) / (B / piece), "%zu runs of %lld pieces for %d", runs.size(), B / piece,
          n_pieces);
}

// the simulator and the scenario sampler
static void check_sim(const PmlForest& f, int depth, long long B) {
    PmlSimWindowPlan P;
    const std::string bad = pml_plan_sim_window(f, depth, B, P);
    CHECK(bad.empty(), "refused: %s", bad.c_str());
    if (!bad.empty()) return;
    const int L = (int)f.td_offsets.size() - 1;
    std::vector<int> size((size_t)f.N, 1), node_depth((size_t)f.N, 0);
    for (int n = f.N - 1; n >= 0; --n)
        if (f.parent[n] >= 0) size[(size_t)f.parent[n]] += size[(size_t)n];
    for (int d = 0; d < L; ++d)
        for (int n = f.td_offsets[d]; n < f.td_offsets[d + 1]; ++n) node_depth[(size_t)n] = d;
    // the frontier: moved down exactly as far as a subtree exceeds B
    CHECK(P.depth >= depth && P.depth <= L, "frontier %d for %d asked, %d levels", P.depth, depth, L);
    for (int d = depth; d <= std::min(P.depth, L - 1); ++d) {
        int most = 0;
        for (int n = f.td_offsets[d]; n < f.td_offsets[d + 1]; ++n) most = std::max(most, size[(size_t)n]);
        if (d < P.depth) CHECK(most > B, "the frontier passed depth %d whose largest subtree holds %d <= %lld nodes", d, most, B);
        else CHECK(most <= B, "a subtree of %d nodes at the frontier %d for a window of %lld", most, d, B);
    }
    std::vector<int> built((size_t)f.N, 0), read((size_t)f.N, 0);
    size_t build_at = 0;
    int at = 0;
    // level runs: consecutive nodes of one depth, in order, all nodes above the frontier
    for (const PmlSimWindowRun& r : P.levels) {
        CHECK(r.first == at && r.count > 0, "level run at %d, expected %d (count %d)", r.first, at, r.count);
        if (r.count <= 0) return;
        at = r.first + r.count;
        const int d = node_depth[(size_t)r.first];
        CHECK(at <= f.td_offsets[d + 1], "a level run crosses the end of depth %d", d);
        if (d == 0) {
            CHECK(r.build_count == 0, "a run of roots builds %d branches", r.build_count);
        } else {
            CHECK(r.build_count == r.count && r.count <= B, "a level run of %d nodes builds %d, window %lld", r.count, r.build_count, B);
            CHECK((size_t)r.build_first == build_at, "level run builds from %d, the list is at %zu", r.build_first, build_at);
            build_at += (size_t)r.build_count;
            for (int i = 0; i < r.build_count; ++i) {
                const int n = P.order[(size_t)(r.build_first + i)];
                CHECK(n == r.first + i, "slot %d of a level run holds node %d, the launch reads %d there", i, n, r.first + i);
                ++built[(size_t)n];
            }
        }
        for (int n = r.first; n < r.first + r.count; ++n) ++read[(size_t)n];
    }
    CHECK(at == f.td_offsets[P.depth], "the level runs end at node %d, the frontier begins at %d", at, f.td_offsets[P.depth]);
    CHECK((size_t)P.list_base == build_at, "the subtrees begin at %d, the level lists end at %zu", P.list_base, build_at);
    // groups: consecutive whole subtrees in preorder, the slot of an entry its position in the group
    const int n_sub = P.depth < L ? f.td_offsets[P.depth + 1] - f.td_offsets[P.depth] : 0;
    CHECK((int)P.sub_off.size() == n_sub + 1 && P.sub_off[0] == 0, "%zu offsets for %d subtrees", P.sub_off.size(), n_sub);
    if ((int)P.sub_off.size() != n_sub + 1) return;
    CHECK(P.order.size() == (size_t)P.list_base + (size_t)P.sub_off.back(), "the list holds %zu entries, the offsets say %d + %d",
          P.order.size(), P.list_base, P.sub_off.back());
    for (int s = 0; s < n_sub; ++s) {
        const int root = f.td_offsets[P.depth] + s, a = P.list_base + P.sub_off[(size_t)s], b = P.list_base + P.sub_off[(size_t)s + 1];
        CHECK(b - a == size[(size_t)root] && P.order[(size_t)a] == root, "subtree %d lists %d entries from node %d, it holds %d below %d", s,
              b - a, P.order[(size_t)a], size[(size_t)root], root);
        std::vector<char> seen((size_t)f.N, 0);   // preorder: a node's parent comes before it, inside the same list
        for (int q = a; q < b; ++q) {
            const int n = P.order[(size_t)q];
            if (q > a) CHECK(f.parent[n] >= 0 && seen[(size_t)f.parent[n]], "node %d of subtree %d is listed before its parent", n, s);
            seen[(size_t)n] = 1;
        }
    }
    int sub_at = 0;
    for (const PmlSimWindowRun& g : P.groups) {
        CHECK(g.first == sub_at && g.count > 0, "group at subtree %d, expected %d (count %d)", g.first, sub_at, g.count);
        if (g.count <= 0 || g.first + g.count > n_sub) return;
        sub_at = g.first + g.count;
        CHECK(g.build_first == P.list_base + P.sub_off[(size_t)g.first] &&
                  g.build_count == P.sub_off[(size_t)sub_at] - P.sub_off[(size_t)g.first],
              "a group builds %d + %d, its subtrees are %d + %d: a subtree is split", g.build_first, g.build_count,
              P.list_base + P.sub_off[(size_t)g.first], P.sub_off[(size_t)sub_at] - P.sub_off[(size_t)g.first]);
        CHECK(g.build_count <= B, "a group of %d entries overflows a window of %lld", g.build_count, B);
        if (sub_at < n_sub)   // greedy: the next subtree did not fit
            CHECK((long long)P.sub_off[(size_t)sub_at + 1] - P.sub_off[(size_t)g.first] > B, "a group was closed early at subtree %d", sub_at);
        for (int i = 0; i < g.build_count; ++i) {
            const int n = P.order[(size_t)(g.build_first + i)];
            ++built[(size_t)n];
            ++read[(size_t)n];
        }
    }
    CHECK(sub_at == n_sub, "the groups end at subtree %d of %d", sub_at, n_sub);
    for (int n = 0; n < f.N; ++n) {
        CHECK(read[(size_t)n] == 1, "node %d is drawn %d times", n, read[(size_t)n]);
        if (f.parent[n] >= 0) CHECK(built[(size_t)n] == 1, "branch %d is built %d times", n, built[(size_t)n]);
        else CHECK(built[(size_t)n] == (P.depth == 0 ? 1 : 0), "root %d is built %d times", n, built[(size_t)n]);   // (harmlessly, in a group)
    }
    const long long launches = (long long)P.levels.size() + (long long)P.groups.size();
    CHECK(launches <= (long long)L + (f.N + B - 1) / B + (long long)P.groups.size(), "%lld launches for %d levels, %d nodes, window %lld",
          launches, L, f.N, B);
    CHECK((long long)P.groups.size() <= 2 * ((f.N + B - 1) / B) + 1, "%zu groups", P.groups.size());   // (two neighbours exceed B)
}

// the sampled counts: the level runs of the top-down sweep's window plan cover every parent once, in order
static void check_counts(const PmlForest& f, const std::vector<int>& bu_order, const std::vector<int>& td_parents,
                         const std::vector<PmlLaunch>& plan, long long B) {
    PmlWindowPlan W;
    const std::string bad = pml_plan_pij_window(plan, f, bu_order, td_parents, B, W);
    CHECK(bad.empty(), "refused: %s", bad.c_str());
    if (!bad.empty()) return;
    int at = 0, runs = 0;
    std::vector<int> built((size_t)f.N, 0);
    for (const PmlWindowStep& w : W.steps) {
        if (!(w.launch.op == OP_LEVEL && w.launch.list == L_TD_PLAIN && w.launch.count > 0)) {
            CHECK(w.build_count == 0, "a record that is no level run builds %d branches", w.build_count);
            continue;
        }
        ++runs;
        CHECK(w.launch.first == at, "run at parent %d, expected %d", w.launch.first, at);
        at = w.launch.first + w.launch.count;
        CHECK(w.build_count <= B, "a run of %d branches for a window of %lld", w.build_count, B);
        int i = 0;
        for (int q = w.launch.first; q < at; ++q)
            for (int j = 0; j < f.n_children[td_parents[(size_t)q]]; ++j, ++i) {
                const int ch = f.first_child[td_parents[(size_t)q]] + j;
                CHECK(i < w.build_count && W.branches[(size_t)(w.build_first + i)] == ch && W.slot[(size_t)ch] == i,
                      "child %d of a run is not in slot %d of its build", ch, i);
                ++built[(size_t)ch];
            }
        CHECK(i == w.build_count, "a run builds %d branches, its parents have %d children", w.build_count, i);
    }
    CHECK(at == (int)td_parents.size(), "the runs cover %d of %zu parents", at, td_parents.size());
    for (int n = 0; n < f.N; ++n) CHECK(built[(size_t)n] == (f.parent[n] >= 0 ? 1 : 0), "branch %d is built %d times", n, built[(size_t)n]);
    const int L = (int)f.td_offsets.size() - 1;
    CHECK(runs <= L + (f.N + B - 1) / B + f.N / std::max<long long>(1, B - pml_window_max_fanout(f) + 1), "%d runs", runs);
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
    PmlSweepTraits tr = {};
    tr.k = 130; tr.W = 3; tr.Gf = tr.Gt = 64;
    tr.fuse = true;
    tr.n_roots = T.n_roots;
    tr.n_cherries = (int)P.cherries.size();
    tr.waves = 4;
    tr.eig_nb = 1;
    tr.C = tr.sched_cols = 3;
    const std::vector<PmlLaunch> top_down = pml_plan_top_down(f, S, tr, false);
    const int fan = pml_window_max_fanout(f), L = (int)f.td_offsets.size() - 1;
    char what[256];
    for (long long B : {(long long)fan, 200ll, (long long)f.N}) {
        snprintf(what, sizeof(what), "%s B=%lld pieces", name, B);
        g_case = what;
        check_pieces(f.N, 128, B);
        check_pieces(f.N, 128, std::max(128ll, B));   // (what the call does below one piece: a window of one piece of its own)
        snprintf(what, sizeof(what), "%s B=%lld counts", name, B);
        g_case = what;
        if (B >= fan) check_counts(f, bu_order, td_parents, top_down, B);
        for (int depth : {0, 3, 16, L}) {
            if (depth > L) continue;
            snprintf(what, sizeof(what), "%s B=%lld frontier %d", name, B, depth);
            g_case = what;
            check_sim(f, depth, B);
        }
    }
    g_case = std::string(name) + " refusals";
    PmlSimWindowPlan none;
    CHECK(!pml_plan_sim_window(f, 0, 0, none).empty(), "a window of no branches was accepted");
    CHECK(!pml_plan_sim_window(f, L + 1, fan, none).empty(), "a frontier below the last level was accepted");
}

int main() {
    run_forest("balanced", grow({256}, split_even));
    run_forest("caterpillar", grow({300}, split_comb));
    run_forest("star", grow({40}, split_star));
    run_forest("ragged forest", grow({400, 1, 150}, split_ragged));
    if (g_failures) {
        printf("%d failures\n", g_failures);
        return 1;
    }
    printf("OK\n");
    return 0;
}
