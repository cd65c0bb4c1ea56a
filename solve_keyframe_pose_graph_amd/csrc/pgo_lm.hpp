// pgo_lm.hpp — the Levenberg-Marquardt controller's state and decisions, host only: Ceres' trust-region rules (trust_region_minimizer.cc / levenberg_marquardt_strategy.cc;
// SURVEY.md Appendix B) and the PCG's pause policy as functions of (LmState, pgo_options, plain scalars) that touch nothing else.  lm_step (pgo_solver.hip) is the sequence of
// these calls around the device work; tests/native/lm_host.cpp instantiates them without a GPU (tests/test_lm_controller.py).  No HIP include: a plain host compiler reads it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "pgo.h"

namespace pgo {

// What the controller carries from one step of a solve to the next (solve_begin: lm_begin, then the first linearisation's x_cost, x_norm, gmax)
struct LmState {
    double radius = 0, decrease_factor = 2, x_cost = 0, x_norm = 0, gmax = 0;
    double last_rho = 1.0;               // relative decrease of the last accepted step of this solve
    bool reuse_diagonal = false, terminated = false, have_prev_step = false;
    int iteration = 0, invalid = 0;      // LM iterations of this solve; consecutive invalid steps
};

inline LmState lm_begin(const pgo_options& o) { LmState s; s.radius = o.initial_trust_region_radius; return s; }

// "A rejection is in the air": the previous step was rejected (rejections come in streaks: the radius shrinks over several steps), or the last accepted step's relative decrease
// fell below 0.8 — the quadratic model is losing its grip (C3's and C4's first rejected steps follow rho = 0.67 and 0.62; the accepted hard steps of both follow rho >= 0.89).
// build_system defers the multigrid of a hard system by it, lm_pause_plan arms both pauses of the PCG by it (a deferred build waits for the first of them).
inline bool rejection_likely(const LmState& s) { return s.reuse_diagonal || s.last_rho < 0.8; }

// a reason to stop; message == nullptr: none, the minimiser goes on
struct LmStop { int type; const char* message; };

// FinalizeIterationAndCheckIfMinimizerCanContinue, before a step
inline LmStop lm_pre_step(const LmState& s, const pgo_options& o, bool ignore_termination) {
    if (ignore_termination) return {PGO_NO_CONVERGENCE, nullptr};
    if (s.iteration >= o.max_num_iterations) return {PGO_NO_CONVERGENCE, "Maximum number of iterations reached."};
    if (s.gmax <= o.gradient_tolerance) return {PGO_CONVERGENCE, "Gradient tolerance reached."};
    if (s.radius < o.min_trust_region_radius) return {PGO_CONVERGENCE, "Minimum trust region radius reached."};
    return {PGO_NO_CONVERGENCE, nullptr};
}

// The PCG pauses at up to two intermediate tolerances (cg_early_tolerance > cg_mid_tolerance > cg_rel_tolerance).  A rejected step
// only changes the trust-region radius (Ceres StepRejected), so a step that is already clearly bad at a pause
// (relative_decrease below the stage's threshold, and neither convergence test would fire: lm_clear_reject) is rejected without paying for the
// remaining decades; otherwise the same PCG resumes towards the next tolerance.
struct LmPauseStage { double tol, reject_rho; };
struct LmPausePlan { int n = 0; LmPauseStage stage[2]; };

// n_keyframes: the caller's count (N_global); cg_predicted: block-Jacobi-equivalent iterations predicted for this system, 0: none; unsuccessful_steps: of this solve so far
inline LmPausePlan lm_pause_plan(const LmState& s, const pgo_options& o, int64_t n_keyframes, double cg_predicted, int unsuccessful_steps) {
    // A pause costs one candidate evaluation (~0.1 ms: eight small launches and a host sync) and pays only when a step is rejected on a system whose PCG is expensive.  The
    // reference's own sessions (hundreds to a few thousand keyframes, steps accepted almost throughout, PCGs of 20-100 iterations at ~14 us) only pay: measured 20.8 -> 17.1 ms
    // on a 400-keyframe trigger, 63.2 -> 60.3 ms at 3 000.  So below CG_PAUSE_MIN_KEYFRAMES the pauses are armed by the first rejected step of the solve (a rejection is
    // usually followed by more: the radius shrinks in several steps) — a rule that depends on the solve's own history only.
    constexpr int64_t CG_PAUSE_MIN_KEYFRAMES = 20000;
    // ... and (round 5) in proportion to what they can save.  A pause costs ~0.25 ms (candidate evaluation, host round trips, the PCG's restart out of its hipGraph), and a
    // system whose step is ACCEPTED pays it for nothing: 13 of C3's 20 steps, 2.8 % of its headline.
    //   * both pauses where a rejection is in the air (rejection_likely: the rule build_system defers the multigrid by);
    //   * the FIRST pause alone, as cheap insurance, where the system is expensive enough for one wasted solve to outweigh dozens of pauses: predicted block-Jacobi-equivalent
    //     iterations x keyframes >= 5.6e7, i.e. a solve of >= ~20 ms (a pause pair is 0.5 ms; a block-Jacobi iteration costs ~36 us per 100 000 keyframes).  rho does NOT
    //     predict every rejection: C5's step 8 follows rho = 0.97 and is rejected with rho = -2.0 — 1.87 s of PCG thrown away against 0.25 s with the pause
    //     (profiles/r05_pause_rule.txt); a system without a prediction counts as mg_switch_iterations iterations;
    //   * none elsewhere.  The PCG's own iterates do not depend on where it pauses.
    const double predicted_its = cg_predicted > 0.0 ? cg_predicted : (double)(o.mg_switch_iterations > 0 ? o.mg_switch_iterations : 400);
    const bool expensive = predicted_its * (double)n_keyframes >= 5.6e7;
    const bool armed = n_keyframes >= CG_PAUSE_MIN_KEYFRAMES || unsuccessful_steps > 0;
    const bool pauses = armed && (rejection_likely(s) || o.cg_pause_always != 0);
    const bool early_only = armed && !pauses && expensive;
    LmPausePlan plan;
    if ((pauses || early_only) && o.cg_early_tolerance > o.cg_rel_tolerance) plan.stage[plan.n++] = LmPauseStage{o.cg_early_tolerance, o.cg_early_reject_rho};
    if (pauses && o.cg_mid_tolerance > o.cg_rel_tolerance && (plan.n == 0 || o.cg_mid_tolerance < plan.stage[0].tol)) plan.stage[plan.n++] = LmPauseStage{o.cg_mid_tolerance, o.cg_mid_reject_rho};
    return plan;
}

// the candidate point x (+) delta as the controller sees it: its cost, the model's cost change and the step's norm
struct LmCandidate { double cost, model_cost_change, step_norm; };

// at a pause: the step is already clearly bad, and neither convergence test would fire on it
inline bool lm_clear_reject(const LmState& s, const pgo_options& o, const LmCandidate& c, double reject_rho) {
    const double mc = c.model_cost_change, dc = s.x_cost - c.cost;
    return mc > 0.0 && std::isfinite(mc) && std::isfinite(c.cost) && dc / mc < reject_rho &&
           c.step_norm > o.parameter_tolerance * (s.x_norm + o.parameter_tolerance) && std::fabs(dc) > o.function_tolerance * s.x_cost;
}

enum class LmOutcome { invalid, invalid_terminal, converged_parameter, converged_function, accepted, rejected };

// How a step ends.  why_invalid: PGO_STEP_ACCEPTED after a valid linear solve (`c` is its candidate), else the pgo_iteration.reason of the invalid step (no candidate was
// evaluated); rejected_at_pause: lm_clear_reject said so, `c` is the candidate of that pause.  Fills step_is_valid, step_is_successful, reason, model_cost_change, step_norm,
// cost_change and relative_decrease of the record.
inline LmOutcome lm_step_outcome(const LmState& s, const pgo_options& o, bool ignore_termination, int why_invalid, bool rejected_at_pause, const LmCandidate& c, pgo_iteration* it) {
    if (why_invalid == PGO_STEP_ACCEPTED) it->model_cost_change = c.model_cost_change;
    if (why_invalid == PGO_STEP_ACCEPTED && (!(c.model_cost_change > 0.0) || !std::isfinite(c.model_cost_change))) why_invalid = PGO_STEP_INVALID_MODEL;
    it->step_is_valid = why_invalid == PGO_STEP_ACCEPTED; it->reason = why_invalid;
    if (!it->step_is_valid)      // HandleInvalidStep
        return s.invalid + 1 >= o.max_num_consecutive_invalid_steps && !ignore_termination ? LmOutcome::invalid_terminal : LmOutcome::invalid;
    it->step_norm = c.step_norm; it->cost_change = s.x_cost - c.cost;
    it->relative_decrease = it->cost_change / it->model_cost_change;
    const bool by_parameter = it->step_norm <= o.parameter_tolerance * (s.x_norm + o.parameter_tolerance);
    const bool by_function = std::fabs(it->cost_change) <= o.function_tolerance * s.x_cost;
    if (!ignore_termination && (by_parameter || by_function)) { it->reason = PGO_STEP_CONVERGED; return by_parameter ? LmOutcome::converged_parameter : LmOutcome::converged_function; }
    it->step_is_successful = std::isfinite(c.cost) && it->relative_decrease > o.min_relative_decrease;
    if (it->step_is_successful) return LmOutcome::accepted;      // HandleSuccessfulStep
    it->reason = rejected_at_pause ? PGO_STEP_REJECTED_AT_PAUSE : PGO_STEP_REJECTED_RHO;
    return LmOutcome::rejected;
}

// the outcomes that end the minimiser
inline LmStop lm_outcome_stop(LmOutcome out) {
    if (out == LmOutcome::invalid_terminal) return {PGO_FAILURE, "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps."};
    if (out == LmOutcome::converged_parameter) return {PGO_CONVERGENCE, "Parameter tolerance reached."};      // (tested before the function tolerance)
    if (out == LmOutcome::converged_function) return {PGO_CONVERGENCE, "Function tolerance reached."};
    return {PGO_NO_CONVERGENCE, nullptr};
}

// The state after a step that ended with `out`: LevenbergMarquardtStrategy::StepIsInvalid / StepRejected / StepAccepted (new_cost: the cost of the relinearisation at the
// accepted point).  A terminal invalid step counts and leaves the radius; a step that converged changes nothing but the count of invalid steps, which every valid step ends.
inline void lm_finish_step(LmState& s, const pgo_options& o, LmOutcome out, double rho, double new_cost) {
    s.invalid = (out == LmOutcome::invalid || out == LmOutcome::invalid_terminal) ? s.invalid + 1 : 0;
    if (out == LmOutcome::invalid) { s.radius *= 0.5; s.reuse_diagonal = true; }
    if (out == LmOutcome::rejected) { s.radius = s.radius / s.decrease_factor; s.decrease_factor *= 2.0; s.reuse_diagonal = true; }
    if (out != LmOutcome::accepted) return;
    s.x_cost = new_cost; s.last_rho = rho;
    s.radius = s.radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3));
    s.radius = std::min(o.max_trust_region_radius, s.radius);
    s.decrease_factor = 2.0; s.reuse_diagonal = false;
}

}  // namespace pgo
