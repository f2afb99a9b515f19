// Host-only check of one fact of pastml_amd/csrc/pml_results.h: "the unit-vector rows of all observed tips of all columns are in the
// posterior table and match the current masks" (PmlResults::tip_rows_kept), which lets a top-down sweep of the F81 family with one
// mask word leave those stores out.  The entries of the library that touch the fact are played to the record the way pml_api.hip
// plays them (begin_top_down, note_top_down, end_top_down and the calls of tip_rows_unknown), and next to it a log of what
// happened is kept.  After every step of every sequence of LENGTH entries the record must answer what the log says:
//     kept  <=>  since the last clearing event, a qualifying sweep was waited for and its bad-tip word was clear
// where a clearing event is an allocation, a write of the masks, a change of the model kind, of an option or of a tunable, a sweep
// of another kernel family (or with the rows left implicit), a sweep whose bad-tip word came back raised, and a pass that returned
// an error.  Two invariants on top: a sweep enqueued with the skip word set implies that the fact held -- by the record and by the
// log -- when it was enqueued, and the option that leaves the rows out of memory being on implies that the fact is not set.
// Prints the number of sequences.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../pastml_amd/csrc/pml_results.h"

static const int LENGTH = 5;

// ---- the log
enum What : char { CLEARED, SWEEP_CLEAN };
struct Log {
    char what[4 * LENGTH + 4];
    int n = 0;
    void add(What w) { what[n++] = w; }
    bool kept() const {
        int last_clear = -1;
        for (int i = 0; i < n; ++i)
            if (what[i] == CLEARED) last_clear = i;
        for (int i = last_clear + 1; i < n; ++i)
            if (what[i] == SWEEP_CLEAN) return true;
        return false;
    }
};

// ---- the context as far as the fact goes, and the entries as pml_api.hip plays them
struct Api {
    PmlResults r;
    bool f81_one_word;   // ctx->kind == PML_MODEL_F81 && ctx->W == 1
    bool implicit;       // PML_OPT_IMPLICIT_TIP_POSTERIORS
    bool off_switch;     // PASTML_HIP_NO_KEEP_TIP_ROWS
    bool word = false;   // the last word of the parameter block's mirror: the sweep leaves the observed tips' stores out
    Log log;
    const char* broken = nullptr;   // the first invariant that did not hold
};

static void begin_top_down(Api& c) { c.word = c.r.tip_rows_kept() && !c.off_switch && !c.implicit && c.f81_one_word; }
static long long n_skipping = 0;
// a top-down sweep goes on the stream
static void note_top_down(Api& c, bool stored) {
    if (c.word) ++n_skipping;
    if (c.word && !c.r.tip_rows_kept()) c.broken = "a sweep was enqueued in skip mode and the record does not hold the fact";
    if (c.word && !c.log.kept()) c.broken = "a sweep was enqueued in skip mode and the rows do not stand";
    if (c.word && (c.implicit || !c.f81_one_word)) c.broken = "skip mode outside the F81 kernels of one mask word";
    c.r.top_down_submitted(stored, c.implicit && c.f81_one_word, c.f81_one_word);
    if (!(c.f81_one_word && !c.implicit)) c.log.add(CLEARED);   // another family writes every row, its bits are not assumed
}
// the wait every top-down entry ends in; raised: what the kernels left in the bad-tip word (only the F81 kernels raise it)
static void end_top_down(Api& c, bool raised) {
    const bool qualifying = c.f81_one_word && !c.implicit;
    raised = raised && c.f81_one_word;
    c.r.top_down_waited(raised);
    if (qualifying) c.log.add(raised ? CLEARED : SWEEP_CLEAN);
}
static void note_bottom_up(Api& c) { c.r.bottom_up_submitted(true, c.f81_one_word, true, false, true, false, false); }

static void chars_alloc(Api& c) {
    c.r.inputs_changed();
    c.r.tip_rows_unknown();
    c.word = false;   // (the mirror is allocated zeroed)
    c.log.add(CLEARED);
}
static void masks_written(Api& c) {   // pml_masks_upload, pml_masks_from_tip_states
    c.r.tip_rows_unknown();
    c.r.inputs_changed();
    c.log.add(CLEARED);
}
static void select_states(Api& c) {
    if (!c.r.posteriors_exist()) return;   // refused
    if (c.r.tip_posteriors_missing()) c.r.tip_posteriors_written();
    c.r.tip_rows_unknown();
    c.r.masks_selected();
    c.log.add(CLEARED);
}
static void set_parameters(Api& c) { c.r.inputs_changed(); }   // set_common, same kind: the rows do not depend on them
static void set_kind(Api& c) {
    c.f81_one_word = !c.f81_one_word;
    c.r.tip_rows_unknown();
    c.r.inputs_changed();
    c.log.add(CLEARED);
}
static void set_option_implicit(Api& c) {
    c.implicit = !c.implicit;
    c.r.tip_rows_unknown();
    c.log.add(CLEARED);
}
static void set_tunable(Api& c, bool the_off_switch) {
    if (the_off_switch) c.off_switch = !c.off_switch;
    c.r.inputs_changed();
    c.r.tip_rows_unknown();
    c.log.add(CLEARED);
}
static void bottom_up(Api& c) {
    c.r.no_results();
    note_bottom_up(c);
    c.r.bottom_up_collected(true);
}
static void top_down_marginals(Api& c, bool raised) {
    if (!c.r.has_marginal()) return;   // refused
    begin_top_down(c);
    note_top_down(c, !c.f81_one_word);
    end_top_down(c, raised);
}
// path 0: both sweeps enqueued, 1: captured as one graph just now, 2: that graph replayed
static void marginal_pass(Api& c, int path, bool ok, bool raised) {
    begin_top_down(c);
    if (path != 2) c.r.no_results();
    for (int i = 0; i < (path == 1 ? 2 : 1); ++i) {   // (captured just now: noted inside the capture and behind it)
        note_bottom_up(c);
        note_top_down(c, !c.f81_one_word);
    }
    end_top_down(c, raised);
    if (ok) {
        c.r.bottom_up_collected(true);
    } else {
        c.r.no_results();
        c.r.tip_rows_unknown();
        c.log.add(CLEARED);
    }
}
static void materialize_td(Api& c, bool raised) {
    if (!c.r.has_top_down()) return;   // refused
    if (c.r.td_vectors_missing()) {
        begin_top_down(c);
        note_top_down(c, true);
        end_top_down(c, raised);
    }
    if (c.r.td_fill_missing()) c.r.td_fill_written();
}

// ---- the alphabet
enum Entry {
    CHARS_ALLOC, MASKS_UPLOAD, MASKS_FROM_TIP_STATES, SELECT_STATES, SET_PARAMETERS, SET_KIND, SET_OPTION, SET_TUNABLE, BOTTOM_UP,
    TOP_DOWN, MARGINAL_PASS, MATERIALIZE_TD, N_ENTRIES
};
struct Event {
    Entry entry;
    int path;    // MARGINAL_PASS
    bool a, b;   // the entry's booleans, in the order of its line in step()
};

static void step(Api& c, const Event& e) {
    switch (e.entry) {
        case CHARS_ALLOC: chars_alloc(c); break;
        case MASKS_UPLOAD: masks_written(c); break;
        case MASKS_FROM_TIP_STATES: masks_written(c); break;
        case SELECT_STATES: select_states(c); break;
        case SET_PARAMETERS: set_parameters(c); break;
        case SET_KIND: set_kind(c); break;
        case SET_OPTION: set_option_implicit(c); break;
        case SET_TUNABLE: set_tunable(c, e.a); break;               // a: it is the off switch
        case BOTTOM_UP: bottom_up(c); break;
        case TOP_DOWN: top_down_marginals(c, e.a); break;           // a: the bad-tip word came back raised
        case MARGINAL_PASS: marginal_pass(c, e.path, e.a, e.b); break;   // a: no error; b: the bad-tip word came back raised
        case MATERIALIZE_TD: materialize_td(c, e.a); break;         // a: the bad-tip word came back raised
        case N_ENTRIES: break;
    }
}

static std::vector<Event> alphabet() {
    static const int n_bools[N_ENTRIES] = {0, 0, 0, 0, 0, 0, 0, 1, 0, 1, 2, 1};
    std::vector<Event> all;
    for (int entry = 0; entry < N_ENTRIES; ++entry)
        for (int path = 0; path < (entry == MARGINAL_PASS ? 3 : 1); ++path)
            for (int bits = 0; bits < (1 << n_bools[entry]); ++bits)
                all.push_back({(Entry)entry, path, (bits & 1) != 0, (bits & 2) != 0});
    return all;
}

static const char* differ(const Api& c) {
    if (c.broken) return c.broken;
    if (c.r.tip_rows_kept() != c.log.kept()) return "tip_rows_kept differs from the log";
    if (c.implicit && c.r.tip_rows_kept()) return "the rows are left out of memory and counted as kept";
    return nullptr;
}

static const std::vector<Event> kEvents = alphabet();
static long long n_sequences = 0;
static int trail[LENGTH];

static void walk(const Api& c, int depth) {
    if (depth == LENGTH) {
        ++n_sequences;
        return;
    }
    for (size_t i = 0; i < kEvents.size(); ++i) {
        Api c2 = c;
        trail[depth] = (int)i;
        step(c2, kEvents[i]);
        if (const char* what = differ(c2)) {
            printf("FAIL: %s after", what);
            for (int d = 0; d <= depth; ++d) {
                const Event& e = kEvents[trail[d]];
                printf(" [entry %d path %d %d%d]", (int)e.entry, e.path, e.a, e.b);
            }
            printf("\n");
            exit(1);
        }
        walk(c2, depth + 1);
    }
}

int main() {
    for (int cfg = 0; cfg < 8; ++cfg) {
        Api c;
        c.f81_one_word = (cfg & 1) != 0;
        c.implicit = (cfg & 2) != 0;
        c.off_switch = (cfg & 4) != 0;
        if (differ(c)) {
            printf("FAIL: a fresh record holds the fact\n");
            return 1;
        }
        walk(c, 0);
    }
    if (n_skipping == 0) {
        printf("FAIL: no sweep was ever enqueued in skip mode\n");
        return 1;
    }
    printf("OK: %lld sequences of %d entries (%zu entries with their arguments, 8 kinds of context), %lld sweeps in skip mode\n",
           n_sequences, LENGTH, kEvents.size(), n_skipping);
    return 0;
}
