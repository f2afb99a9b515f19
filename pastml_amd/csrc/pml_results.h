// What the result buffers of a context hold: which sweeps' results are valid, which rows a sweep left in registers only, whether
// P(t) is that of the current parameters.  Every C entry asks it whether it may run and what it has to write first, and tells it
// what it put on the stream.  Plain C++ (no HIP, no pml_ctx): tests/results_driver.cpp walks it on the host against the flag
// writes it replaced.
#pragma once

struct PmlResults {
    // ---- may this call run?
    bool has_marginal() const { return bu_mode == 1; }   // a collected bottom-up sweep, marginal
    bool has_joint() const { return bu_mode == 0; }      // ... joint
    bool has_bottom_up() const { return bu_mode >= 0; }
    bool has_top_down() const { return td_valid; }
    bool has_joint_states() const { return js_valid; }
    bool posteriors_exist() const { return post_ever; }      // of some earlier top-down sweep, still in memory
    bool joint_states_exist() const { return js_ever; }      // of some earlier back-trace
    // ---- what was left out of memory?
    bool pij_stale() const { return prep_dirty; }            // P(t) / exp(-mu t') is not that of the parameters
    bool cherries_missing() const { return bu_fused; }       // the last bottom-up sweep kept the cherries' vectors in registers
    bool cherries_joint() const { return bu_fused_joint; }   // ... and it was a joint sweep
    bool children_missing() const { return bu_absorbed; }    // ... and the children of the two-level and stacked units
    bool td_vectors_missing() const { return !td_vec_valid; }  // the last top-down sweep ran without the TD stores
    bool td_fill_missing() const { return !td_filled; }      // the TD vectors of the nodes no sweep stores (td_fill_kernel)
    bool tip_posteriors_missing() const { return tip_post_missing; }  // the observed tips' rows were left implicit
    // ---- what may a sweep leave alone?
    // The unit-vector rows of ALL observed tips of ALL columns are in the posterior table and match the current masks: a top-down
    // sweep of the F81 family with one mask word need not store them again (they depend on the masks and on nothing else).
    bool tip_rows_kept() const { return tip_rows; }

    // ---- inputs
    // masks, model parameters, columns, the eigen options, any tunable: P(t) is stale and no sweep's result stands
    void inputs_changed() {
        prep_dirty = true;
        no_results();
    }
    // the initial masks: only the joint sweep's tables read them, so a back-trace needs a new sweep; P(t) and what finished sweeps
    // delivered do not depend on them
    void initial_masks_changed() { bu_mode = -1; }
    // a selection rewrote the masks: sweeps must be redone, the posteriors and joint states it read stay valid for inspection
    void masks_selected() {
        prep_dirty = true;
        bu_mode = -1;
    }
    // batch or window: P(t) is rebuilt from the other source; the sweeps' results do not depend on where it came from
    void pij_source_changed() { prep_dirty = true; }
    void pij_built() { prep_dirty = false; }

    // ---- sweeps
    // A bottom-up sweep is on the stream (enqueued or replayed); nothing is valid until it is collected.  ran_batch: it built the
    // batch of P(t); some_columns: not every column took part -- where an earlier sweep left the children of the others' units
    // out of memory they still are (rebuilding rows that are in memory is harmless).
    void bottom_up_submitted(bool marginal, bool f81, bool cherries, bool two_level, bool ran_batch, bool some_columns,
                             bool fused_joint) {
        no_results();
        if (ran_batch) prep_dirty = false;
        bu_fused_joint = fused_joint;
        bu_fused = (marginal && f81 && cherries) || fused_joint;
        bu_absorbed = (marginal && f81 && two_level) || (some_columns && bu_absorbed);
    }
    void bottom_up_collected(bool marginal) { bu_mode = marginal ? 1 : 0; }   // (not on zero likelihood)
    // A top-down sweep is on the stream.  vectors_stored: with the TD stores; tips_implicit: observed tips' posteriors left out
    // of memory; f81_one_word: by the kernels of the F81 family with one mask word, which write an observed tip's row as the unit
    // vector of its mask -- or leave the store out where the row is kept -- and raise the bad-tip word where they write NaNs
    // instead.  Any other family writes every row itself: its bits are not assumed.
    void top_down_submitted(bool vectors_stored, bool tips_implicit, bool f81_one_word) {
        td_valid = post_ever = true;
        td_vec_valid = vectors_stored;
        td_filled = false;
        tip_post_missing = tips_implicit;
        tip_sweep = f81_one_word && !tips_implicit;
        if (!tip_sweep) tip_rows = false;
    }
    void top_down_submitted(bool vectors_stored, bool tips_implicit) { top_down_submitted(vectors_stored, tips_implicit, false); }
    // the host has waited for that sweep and read its bad-tip word: raised = some observed tip's row is NaNs now
    void top_down_waited(bool bad_tip) {
        if (tip_sweep) tip_rows = !bad_tip;
        tip_sweep = false;
    }
    // The observed tips' rows may not stand any more, or not match the masks: the masks were written, the table may have been
    // reallocated, the model kind, an option or a tunable changed, a pass returned an error.  (A change of the model's
    // parameters is none of these: inputs_changed leaves the fact alone.)
    void tip_rows_unknown() { tip_rows = tip_sweep = false; }
    void joint_states_fetched() { js_valid = js_ever = true; }
    // a sweep is about to overwrite the buffers, or a pass found a column without likelihood: nothing in them means anything
    void no_results() {
        bu_mode = -1;
        td_valid = js_valid = false;
    }

    // ---- lazy materialisations (the TD vectors: a top-down sweep with the stores on, top_down_submitted)
    void cherries_written() { bu_fused = false; }
    void children_written() { bu_absorbed = false; }
    void td_fill_written() { td_filled = true; }
    void tip_posteriors_written() { tip_post_missing = false; }

private:
    int bu_mode = -1;  // -1 invalid, 1 marginal, 0 joint
    bool td_valid = false, js_valid = false;
    bool post_ever = false, js_ever = false;
    bool prep_dirty = true;
    bool bu_fused = false, bu_fused_joint = false, bu_absorbed = false;
    bool td_vec_valid = false, td_filled = false, tip_post_missing = false;
    bool tip_rows = false;    // the observed tips' unit rows stand in the table
    bool tip_sweep = false;   // the sweep on the stream makes that so unless its bad-tip word comes back raised
};
