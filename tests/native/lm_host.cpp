// Host instantiation of the LM controller (csrc/pgo_lm.hpp): one flat entry point over arrays of doubles.  Built as a shared object for tests/test_lm_controller.py, or — with
// -DLM_MAIN — as a stand-alone program that reads the same cases from standard input, one per line, and prints their results: the form to run under
// -fsanitize=address,undefined.
//
// lm_shim(op, in, n_in, out, msg): in = the state (LM_STATE doubles, the order of LmState's fields as listed below), the options the controller reads (LM_OPTIONS doubles),
// then what the operation takes; out = what it gives; *msg = the termination message, "" without one.  Returns the number of doubles written, -1 for a malformed call.
//   begin                                                                   -> state
//   pre     ignore_termination                                              -> stop, termination type
//   plan    keyframes, predicted PCG iterations, unsuccessful steps         -> stages, then (tolerance, reject rho) of each
//   reject  candidate cost, model cost change, step norm; reject rho        -> clear reject
//   step    ignore_termination, why_invalid, rejected at a pause; candidate cost, model cost change, step norm; the cost of the relinearisation
//           -> outcome, state after lm_finish_step, step_is_valid, step_is_successful, reason, model_cost_change, step_norm, cost_change, relative_decrease of the record,
//              rejection_likely of the new state, stop, termination type
#include <cstring>

#include "pgo_lm.hpp"

enum { LM_STATE = 11, LM_OPTIONS = 16 };

static pgo::LmState state_of(const double* v) {
    pgo::LmState s;
    s.radius = v[0]; s.decrease_factor = v[1]; s.x_cost = v[2]; s.x_norm = v[3]; s.gmax = v[4]; s.last_rho = v[5];
    s.reuse_diagonal = v[6] != 0.0; s.terminated = v[7] != 0.0; s.have_prev_step = v[8] != 0.0; s.iteration = (int)v[9]; s.invalid = (int)v[10];
    return s;
}
static int put_state(const pgo::LmState& s, double* v) {
    const double f[LM_STATE] = {s.radius, s.decrease_factor, s.x_cost, s.x_norm, s.gmax, s.last_rho, (double)s.reuse_diagonal, (double)s.terminated, (double)s.have_prev_step, (double)s.iteration, (double)s.invalid};
    std::memcpy(v, f, sizeof(f));
    return LM_STATE;
}
static pgo_options options_of(const double* v) {
    pgo_options o;
    std::memset(&o, 0, sizeof(o));
    o.max_num_iterations = (int32_t)v[0]; o.max_num_consecutive_invalid_steps = (int32_t)v[1]; o.initial_trust_region_radius = v[2]; o.max_trust_region_radius = v[3];
    o.min_trust_region_radius = v[4]; o.min_relative_decrease = v[5]; o.function_tolerance = v[6]; o.gradient_tolerance = v[7]; o.parameter_tolerance = v[8];
    o.cg_rel_tolerance = v[9]; o.cg_early_tolerance = v[10]; o.cg_early_reject_rho = v[11]; o.cg_mid_tolerance = v[12]; o.cg_mid_reject_rho = v[13];
    o.cg_pause_always = (int32_t)v[14]; o.mg_switch_iterations = (int32_t)v[15];
    return o;
}

extern "C" {
int lm_shim_state_doubles() { return LM_STATE; }
int lm_shim_option_doubles() { return LM_OPTIONS; }
int lm_shim(const char* op, const double* in, int n_in, double* out, const char** msg) {
    *msg = "";
    if (n_in < LM_STATE + LM_OPTIONS) return -1;
    pgo::LmState s = state_of(in);
    const pgo_options o = options_of(in + LM_STATE);
    const double* a = in + LM_STATE + LM_OPTIONS;
    const int n = n_in - LM_STATE - LM_OPTIONS;
    auto put_stop = [&](const pgo::LmStop& st, double* v) { v[0] = st.message ? 1.0 : 0.0; v[1] = st.type; if (st.message) *msg = st.message; return 2; };
    if (!std::strcmp(op, "begin") && n == 0) return put_state(pgo::lm_begin(o), out);
    if (!std::strcmp(op, "pre") && n == 1) return put_stop(pgo::lm_pre_step(s, o, a[0] != 0.0), out);
    if (!std::strcmp(op, "plan") && n == 3) {
        const pgo::LmPausePlan P = pgo::lm_pause_plan(s, o, (int64_t)a[0], a[1], (int)a[2]);
        out[0] = P.n;
        for (int k = 0; k < P.n; ++k) { out[1 + 2 * k] = P.stage[k].tol; out[2 + 2 * k] = P.stage[k].reject_rho; }
        return 1 + 2 * P.n;
    }
    if (!std::strcmp(op, "reject") && n == 4) { out[0] = pgo::lm_clear_reject(s, o, pgo::LmCandidate{a[0], a[1], a[2]}, a[3]) ? 1.0 : 0.0; return 1; }
    if (!std::strcmp(op, "step") && n == 7) {
        pgo_iteration it;
        std::memset(&it, 0, sizeof(it));
        const pgo::LmOutcome r = pgo::lm_step_outcome(s, o, a[0] != 0.0, (int)a[1], a[2] != 0.0, pgo::LmCandidate{a[3], a[4], a[5]}, &it);
        pgo::lm_finish_step(s, o, r, it.relative_decrease, a[6]);
        int k = 0;
        out[k++] = (double)(int)r;
        k += put_state(s, out + k);
        for (double v : {(double)it.step_is_valid, (double)it.step_is_successful, (double)it.reason, it.model_cost_change, it.step_norm, it.cost_change, it.relative_decrease}) out[k++] = v;
        out[k++] = pgo::rejection_likely(s) ? 1.0 : 0.0;
        return k + put_stop(pgo::lm_outcome_stop(r), out + k);
    }
    return -1;
}
}

#ifdef LM_MAIN
#include <cstdio>
#include <vector>

// a case per line: the operation, the number of doubles, the doubles; answered by a line of the doubles written (%.17g: they read back to the same bits), then | and the message
int main() {
    char op[16];
    int n_in, cases = 0;
    while (std::scanf("%15s %d", op, &n_in) == 2) {
        if (n_in < 0 || n_in > 64) { std::printf("bad case\n"); return 2; }
        std::vector<double> in((size_t)n_in), out(32);
        for (double& v : in) if (std::scanf("%lf", &v) != 1) { std::printf("bad case\n"); return 2; }
        const char* msg = "";
        const int n = lm_shim(op, in.data(), n_in, out.data(), &msg);
        if (n < 0) { std::printf("bad case\n"); return 2; }
        for (int k = 0; k < n; ++k) std::printf("%.17g ", out[(size_t)k]);
        std::printf("|%s\n", msg);
        ++cases;
    }
    return cases > 0 ? 0 : 2;
}
#endif
