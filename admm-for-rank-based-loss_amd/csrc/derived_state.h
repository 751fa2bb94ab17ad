// derived_state.h - what a solver handle has computed from its inputs and may reuse, and which change of an input voids it.
// Plain C++ (no HIP): the api*.hip units embed Derived in rbl_solver, tests/derived_state_main.cpp prints the table.
//
// The inputs: D (the data matrix -y X), Y (the labels: the owner's y inside D, a borrower's own through rbl_set_labels),
// W, Z, LAM, RHO (the iterate), RW (row weights), G (the Gram matrix) and SWEEP (that the handle runs the single-sweep
// erm iteration on an unbroken chain of rho predictions).  Each flag below vouches for a buffer; `changed` is the one
// place that says which inputs that buffer was computed from.  An entry point that changes an input names its cause
// (data_changed, w_changed, ...) and never picks flags.  The phases (api_iter.hip, api_dist.hip) set the flags where
// they fill the buffers and clear them where they consume them: that is the state machine, not an invalidation.
//
// Not here: rbl_solver::data_ready (D is there at all); the verdict objects, back-off counters, fused_ok, fuse_v and
// in_group (configuration); WstepWorkspace::gw_valid (run_wstep resets it on entry and the driver reads it only right
// behind that call - it never outlives an entry point); spec_w - w holds a w-step enqueued ahead of time - which is
// undone by a device copy, not by a flag: cancel_spec, run by RBL_ENTER in front of every mutator.
#pragma once

struct Derived {
    enum : unsigned { D = 1, Y = 2, W = 4, Z = 8, LAM = 16, RHO = 32, RW = 64, G = 128, SWEEP = 256 };

    // v holds D w.  From D, w (own labels leave v in the owner's sign convention)
    bool v_valid = false;
    // z_next, q and ||z_next||^2 hold the next iteration's z-step and q pass, done ahead by a single-sweep pass for the
    // rho it predicted.  From D, y, w, z, lambda, rho, row weights; only on the single-sweep chain
    bool z_ready = false;
    // p holds D^T lambda, carried from iteration to iteration in d-space.  From D, y, lambda; single-sweep chain
    bool p_valid = false;
    // q's second half holds a fresh D^T lambda that the next w-step copies into p.  From D, y, lambda; single-sweep chain
    bool p_pending = false;
    // pred holds the rho predicted behind the w-step in flight.  From everything q and the residuals come from: D, y, w,
    // z, lambda, rho, row weights, G; single-sweep chain
    bool pred_valid = false;
    // sw.keys[0] / vals[0] hold the 64-bit sort keys of m = D w - lambda/rho and the row ids.  From D, y, w, lambda, rho
    bool keys_ready = false;
    // m and its range (s32.mm) stand ready for the 32-bit keys.  From D, y, w, lambda, rho
    bool s32_m_ready = false;
    // z came from the sort with 32-bit keys and its verdict is unread; a redo re-forms z from m.  From D, y, w, z, lambda, rho
    bool s32_used = false;
    // ... and q was formed from that z already, so a redo owes q as well.  From D, y, w, z, lambda, rho
    bool s32_q_done = false;
    // z came from the sort-free banded z-step and its verdict is unread.  From D, y, w, z, lambda, rho
    bool zb_used = false;
    // ... and q was formed from that z already.  From D, y, w, z, lambda, rho
    bool zb_q_done = false;
    // c holds z + lambda/rho, written by the banded z-step next to z.  From z, lambda, rho
    bool zb_c_ready = false;
    // G holds D^T D of this handle's rows (rbl_gram_local).  From D
    bool gram_local_done = false;
    // G is whole and L was taken from it (rbl_gram_finish).  From D, G
    bool gram_ready = false;
    // ww.eig_* hold the eigenbasis of G (opt-in ridge w-step).  From G
    bool eig_ok = false;

    // the table: every flag whose buffer was computed from one of the inputs in `in` falls
    void changed(unsigned in) {
        const auto dep = [in](bool& flag, unsigned on) {
            if (on & in) flag = false;
        };
        dep(v_valid, D | W);
        dep(z_ready, D | Y | W | Z | LAM | RHO | RW | SWEEP);
        dep(p_valid, D | Y | LAM | SWEEP);
        dep(p_pending, D | Y | LAM | SWEEP);
        dep(pred_valid, D | Y | W | Z | LAM | RHO | RW | G | SWEEP);
        dep(keys_ready, D | Y | W | LAM | RHO);
        dep(s32_m_ready, D | Y | W | LAM | RHO);
        dep(s32_used, D | Y | W | Z | LAM | RHO);
        dep(s32_q_done, D | Y | W | Z | LAM | RHO);
        dep(zb_used, D | Y | W | Z | LAM | RHO);
        dep(zb_q_done, D | Y | W | Z | LAM | RHO);
        dep(zb_c_ready, Z | LAM | RHO);
        dep(gram_local_done, D);
        dep(gram_ready, D | G);
        dep(eig_ok, G);
    }
};

// ---- the causes: what an entry point says it did
// an upload wrote D and the labels in it; the G that stands belongs to the old D
inline void data_changed(Derived& s) { s.changed(Derived::D | Derived::Y | Derived::G); }
inline void w_changed(Derived& s) { s.changed(Derived::W); }
// z was replaced from outside: rbl_set_state between iterations, rbl_phase_z_external inside one
inline void z_replaced(Derived& s) { s.changed(Derived::Z); }
inline void lambda_changed(Derived& s) { s.changed(Derived::LAM); }
inline void rho_changed(Derived& s) { s.changed(Derived::RHO); }
inline void labels_changed(Derived& s) { s.changed(Derived::Y); }
inline void row_weights_changed(Derived& s) { s.changed(Derived::RW); }
// G is being rewritten: by rbl_gram_local (a shard's share until the driver has summed it), then finished
inline void gram_changed(Derived& s) { s.changed(Derived::G); }
// the single-sweep look-ahead is void: the handle leaves the single-sweep iteration (a group, own labels) or a step of
// the chain was skipped (rbl_phase_w_external: no rho prediction, the d-space recurrence did not advance)
inline void drop_look_ahead(Derived& s) { s.changed(Derived::SWEEP); }

// ---- the Gram matrix is formed in two calls on the owner of D; these are their produce sites
inline void gram_formed(Derived& s) {
    gram_changed(s);
    s.gram_local_done = true;
}
inline void gram_finished(Derived& s, bool eigenbasis) {
    s.gram_ready = true;
    s.eig_ok = eigenbasis;
}
