// lm_common.hpp — the one text of what the two refinement kernels (kernels_lm.hip: 15 x 7 register layouts; kernels_lm_any.hip:
// any patch size) run around their residual evaluators: the scalar solver -- Eigen's LevenbergMarquardt<NumericalDiff<...>> for one
// unknown (minimizeInit / minimizeOneStep, MINPACK's lmdif: SURVEY.md Appendix B.1) under the outer loop of
// DepthProblemSolver.cpp:161-188 --, DepthProblem::setProblem's pose, the scale-loop guard's bookkeeping and the epilogue that
// turns a solved match into a point (DepthProblemSolver.cpp:190-244).  (patchInterpolation's geometry stays with each kernel:
// shared in the straight-line form of kernels_lm.hip it doubled the general kernel's SGPR spills and cost it 1 %.)
//
// The solver is a state machine (LmSolver) around ONE call site of the evaluator per kernel: phase 0 is F(x0) of minimizeInit,
// phase 1 F(x + h) of NumericalDiff, phase 2 F(x + p) of the trust-region trial.  A kernel evaluates F(S.xe), reduces the patch
// sums its phase needs its own way (registers and DPP against LDS and shuffles) and hands the scalars to the function of that
// phase; where the residual arrays live, the Jacobian quotients and the copy F(x) <- F(xnew) of an accepted step stay with the
// kernel.  Everything here is inlined: no launch, no memory, no kernel argument of its own.
#pragma once
#include "common.hpp"
#include "dev_hooks.hpp"

namespace esvo {

// internal::lmpar2 for n == 1 (Appendix B.1)
__device__ inline double lm_lmpar2(double r, double diag, double qtf, double delta, double& par) {
  const double dwarf = 2.2250738585072014e-308;
  double x = qtf / r;
  double wa2 = diag * x;
  double dxnorm = fabs(wa2);
  double fp = dxnorm - delta;
  if (fp <= 0.1 * delta) { par = 0; return x; }
  double wa1 = diag * wa2 / dxnorm;
  wa1 = wa1 / r;
  double temp = fabs(wa1);
  double parl = fp / delta / temp / temp;
  wa1 = r * qtf / diag;
  const double gn = fabs(wa1);
  double paru = gn / delta;
  if (paru == 0.) paru = dwarf / ((delta < 0.1) ? delta : 0.1);
  par = (par < parl) ? parl : par;   // std::max(par, parl)
  par = (paru < par) ? paru : par;   // std::min(par, paru)
  if (par == 0.) par = gn / dxnorm;
  int it = 0;
  while (true) {
    ++it;
    if (par == 0.) { const double c = 0.001 * paru; par = (dwarf < c) ? c : dwarf; }
    const double ds = sqrt(par) * diag;
    const double sdiag2 = r * r + ds * ds;
    const double sdiag = sqrt(sdiag2);
    x = r * qtf / sdiag2;
    wa2 = diag * x;
    dxnorm = fabs(wa2);
    temp = fp;
    fp = dxnorm - delta;
    if (fabs(fp) <= 0.1 * delta || (parl == 0. && fp <= temp && temp < 0.) || it == 10) break;
    wa1 = diag * (wa2 / dxnorm);
    wa1 = wa1 / sdiag;
    temp = fabs(wa1);
    const double parc = fp / delta / temp / temp;
    if (fp > 0.) parl = (parl < par) ? par : parl;
    if (fp < 0.) paru = (par < paru) ? par : paru;
    const double pc = par + parc;
    par = (parl < pc) ? pc : parl;
  }
  return x;
}

// ---- the solver ---------------------------------------------------------------------------------------------------------------
constexpr double LM_FTOL = 1e-6, LM_XTOL = 1e-6, LM_GTOL = 0., LM_FACTOR = 100.;
constexpr double LM_EPS = 2.220446049250313e-16;
constexpr double LM_SQRT_EPS = 1.4901161193847656e-08;  // sqrt(DBL_EPSILON), exact

struct LmSolver {
  double x, fnorm, par, diag, xnorm, delta, r, qtf, gnorm;
  double h, xnew, wa1, pnorm;
  double xe;  // the point the evaluator is asked for next
  int nfev, iter, iteration, optState;
  int phase;
  bool need_step;
};
__device__ __forceinline__ void lm_start(LmSolver& S, double x0) {
  S.x = x0;
  S.fnorm = 0.; S.par = 0.; S.diag = 0.; S.xnorm = 0.; S.delta = 0.; S.r = 0.; S.qtf = 0.; S.gnorm = 0.;
  S.h = 0.; S.xnew = 0.; S.wa1 = 0.; S.pnorm = 0.;
  S.nfev = 1; S.iter = 1; S.iteration = 0; S.optState = 0;
  S.phase = 0;
  S.need_step = false;
  S.xe = x0;
}
// NumericalDiff<Forward>'s step at x
__device__ __forceinline__ double lm_diff_step(double x) {
  double h = LM_SQRT_EPS * fabs(x);
  if (h == 0.) h = LM_SQRT_EPS;
  return h;
}
// before the evaluation: the LM parameter and the trial point (minimizeOneStep, inner loop head)
__device__ __forceinline__ void lm_trial_point(LmSolver& S) {
  if (S.need_step) {
    const double pstep = lm_lmpar2(S.r, S.diag, S.qtf, S.delta, S.par);
    S.wa1 = -pstep;
    S.xnew = S.x + S.wa1;
    S.pnorm = fabs(S.diag * S.wa1);
    if (S.iter == 1) S.delta = (S.pnorm < S.delta) ? S.pnorm : S.delta;
    S.xe = S.xnew;
    S.need_step = false;
  }
}
// phase 0, minimizeInit: fnorm = |F(x0)|
__device__ __forceinline__ void lm_after_init(LmSolver& S, double fnorm) {
  S.fnorm = fnorm;
  S.par = 0.;
  S.iter = 1;
}
// phase 1, NumericalDiff<Forward>::df and the head of minimizeOneStep: wa2n = |J|, jtf = J^T F(x), fvec0 = element (0, 0) of
// F(x).  The reference evaluates F(x) again (val1) and F(x + h); F is a pure function and the kernel already holds F(x), so only
// F(x + h) was computed -- nfev still advances by 2 (it drives the maxfev test).  Returns the status: 4, or -1 = go on to the trial.
__device__ __forceinline__ int lm_after_diff(LmSolver& S, double wa2n, double jtf, double fvec0) {
  S.nfev += 2;
  S.r = wa2n;
  S.qtf = (S.r != 0.) ? jtf / S.r : fvec0;
  if (S.iter == 1) {
    S.diag = (wa2n == 0.) ? 1. : wa2n;
    S.xnorm = fabs(S.diag * S.x);
    S.delta = LM_FACTOR * S.xnorm;
    if (S.delta == 0.) S.delta = LM_FACTOR;
  }
  S.gnorm = 0.;
  if (S.fnorm != 0.)
    if (wa2n != 0.) { const double g = fabs(S.r * (S.qtf / S.fnorm) / wa2n); S.gnorm = (S.gnorm < g) ? g : S.gnorm; }
  if (S.gnorm <= LM_GTOL) return 4;
  S.diag = (S.diag < wa2n) ? wa2n : S.diag;
  S.need_step = true;
  S.phase = 2;
  return -1;
}
// phase 2, the trust-region trial at xnew: fnorm1 = |F(xnew)|.  accept() runs where the reference copies wa4 into fvec -- the
// kernel's F(x) <- F(xnew).  Returns whether minimizeOneStep returns (with `status`, or Running = -1); otherwise its inner loop
// goes round again: do { ... } while (ratio < 1e-4).
// (The shape is measured, not a matter of taste: with accept taken by reference the Student-t instances of lm_refine_kernel
// allocate the registers they did with this text written out in the kernel; taken by value, or as a returned flag with the copy
// behind the call, the guarded narrow instance needs 2 to 4 VGPRs more -- profiles/lm_one_driver.txt.)
template <typename ACCEPT>
__device__ __forceinline__ bool lm_after_trial(LmSolver& S, double fnorm1, int maxfev, int& status, ACCEPT&& accept) {
  ++S.nfev;
  double actred = -1.;
  if (0.1 * fnorm1 < S.fnorm) actred = 1. - (fnorm1 / S.fnorm) * (fnorm1 / S.fnorm);
  const double wa3 = S.r * S.wa1;
  const double t1 = fabs(wa3) / S.fnorm, temp1 = t1 * t1;
  const double t2 = sqrt(S.par) * S.pnorm / S.fnorm, temp2 = t2 * t2;
  const double prered = temp1 + temp2 / 0.5;
  const double dirder = -(temp1 + temp2);
  double ratio = 0.;
  if (prered != 0.) ratio = actred / prered;
  if (ratio <= 0.25) {
    double temp = 0.5;
    if (actred >= 0.) temp = 0.5;
    if (actred < 0.) temp = 0.5 * dirder / (dirder + 0.5 * actred);
    if (0.1 * fnorm1 >= S.fnorm || temp < 0.1) temp = 0.1;
    const double pn = S.pnorm / 0.1;
    S.delta = temp * ((pn < S.delta) ? pn : S.delta);
    S.par /= temp;
  } else if (!(S.par != 0. && ratio < 0.75)) {
    S.delta = S.pnorm / 0.5;
    S.par = 0.5 * S.par;
  }
  if (ratio >= 1e-4) {
    S.x = S.xnew;
    accept();
    S.xnorm = fabs(S.diag * S.x);
    S.fnorm = fnorm1;
    ++S.iter;
  }
  if (fabs(actred) <= LM_FTOL && prered <= LM_FTOL && 0.5 * ratio <= 1. && S.delta <= LM_XTOL * S.xnorm) status = 3;
  else if (fabs(actred) <= LM_FTOL && prered <= LM_FTOL && 0.5 * ratio <= 1.) status = 1;
  else if (S.delta <= LM_XTOL * S.xnorm) status = 2;
  else if (S.nfev >= maxfev) status = 5;
  else if (fabs(actred) <= LM_EPS && prered <= LM_EPS && 0.5 * ratio <= 1.) status = 6;
  else if (S.delta <= LM_EPS * S.xnorm) status = 7;
  else if (S.gnorm <= LM_EPS) status = 8;
  if (status >= 0 || !(ratio < 1e-4)) return true;
  S.need_step = true;
  return false;
}
// behind the phase: `returned` = minimizeOneStep returned (status, or -1 = Running), which is one pass of the reference's outer
// loop, DepthProblemSolver.cpp:161-188.  Returns whether the solve is over; otherwise a pass that starts with a Jacobian asks for
// the difference point next.  (Behind phase 0 it is the step from minimizeInit to the first Jacobian: the split launch's second
// stage resumes with lm_after_init + this.)
__device__ __forceinline__ bool lm_next(LmSolver& S, bool returned, int status, int max_iter) {
  if (S.phase == 0) {
    S.phase = 1;
  } else if (returned) {
    S.iteration++;
    if (S.iteration >= max_iter) return true;
    if (status == 2 || status == 3) {
      if (S.optState == 0) S.optState++;
      else return true;
    }
    S.phase = 1;
  }
  if (S.phase == 1) {  // next evaluation: F(x + h) for the forward difference
    S.h = lm_diff_step(S.x);
    S.xe = S.x + S.h;
  }
  return false;
}

// ---- DepthProblem::setProblem, DepthProblem.cpp:17-32: T = T_left_virtual (3 x 4) --------------------------------------------------
__device__ __forceinline__ void lm_set_problem(const LmArgs& a, const esvo_match_t& m, double* T) {
  double Tlw[16], Tlv[16];
  rigid_inverse(a.T_world_obs, Tlw);
  mat4_mul(Tlw, a.pose_T + (size_t)m.pose_idx * 16, Tlv);
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = Tlv[i];
}

// ---- the scale-loop guard (common.hpp: LmGuard) -------------------------------------------------------------------------------------
// What a guarded evaluation reports, uniform over the match's lanes like the scale loop itself: passes = completed updates
// s2 = sum / N with a non-zero sum (0 on the failure fill and on the shortcut), shortcut, and over = the loop had completed `limit`
// passes when its test asked for another -- it ends there, the caller abandons the match.
struct LmGuardEval { int limit, passes; bool shortcut, over; };
// a match's counts over its evaluations
template <bool GUARD> struct LmGuardCounts {};
template <> struct LmGuardCounts<true> {
  int evals = 0, passes = 0, max_eval = 0, shortcut = 0;
  bool abandoned = false;
  __device__ __forceinline__ void add(const LmGuardEval& ge) {
    ++evals;
    passes += ge.passes;
    max_eval = max(max_eval, ge.passes);
    shortcut += ge.shortcut ? 1 : 0;
  }
};

// ---- the epilogue, DepthProblemSolver.cpp:190-244: the match of slot s (index j of the list) solved to x with |J| = r and
// |F(x)| = fnorm over N residuals -> solved test, variance, point, culling, the slot's point and flag.  One lane per match.
template <bool L2>
__device__ __forceinline__ void lm_store_point(const LmArgs& a, const DevParams& p, u32* n_solved, const esvo_match_t& m, u32 s, u32 j,
                                               double x, double r, double fnorm, int N) {
  const bool solved = !(x <= 0.001);  // DepthProblemSolver.cpp:192
  bool keep = solved;
  if (solved) {
    atomicAdd(n_solved, 1u);
    const double invJtJ = (r != 0.) ? (1. / r) * (1. / r) : 0.;  // internal::covar, n == 1
    double variance;
    if constexpr (L2) {  // :200-206: cov = |f|^2 / (values - inputs) * (J^T J)^-1; DepthPoint::update on a new point bounds it
      // (upstream takes lm.fvec.blueNorm() here and lm.fnorm -- stableNorm -- for the residual below: two Eigen algorithms for
      // the same |f| that may round differently in the last place.  Both are third-party code absent from the reference tree;
      // this path and the oracle use the solver's one canonical |f| for both.  Stated deviation, DESIGN.md "Deviations".)
      variance = fnorm * fnorm / (double)(N - 1) * invJtJ;
      if (variance < 1e-6) variance = 1e-6;
    } else {
      variance = p.td_stdvar2 * invJtJ;                          // :210
    }
    const double residual = fnorm * fnorm;                       // :212
    const double cx = m.x_left[0], cy = m.x_left[1];
    DevPoint o;
    o.row = (u32)(size_t)floor(cy);  // :116
    o.col = (u32)(size_t)floor(cx);
    o.x[0] = cx;
    o.x[1] = cy;
    cam2World(p.camL, cx, cy, x, o.p_cam);                       // :119
    DEV_PERTURB_POINT(o, s);  // (empty in the product: dev_hooks.hpp)
    o.inv_depth = x;                                             // update_studentT, new-point branch
    o.scale2 = L2 ? 0.0 : variance * (p.td_nu - 2) / p.td_nu;    // :125 (l2: the Gaussian update leaves scaleSquared_ / nu_
    o.nu = L2 ? 0.0 : p.td_nu;                                   //  as constructed -- zero here and in the oracle, Appendix A-8)
    o.variance = variance;
    o.residual = residual;
    o.age = 0;
    o.pose_idx = m.pose_idx;
    o.seq = j;
    if (a.cull)  // pointCulling, :230-234
      keep = variance <= p.var_thr && residual <= p.cost_thr && x > -1e-6 && x >= p.invdepth_min && x <= p.invdepth_max;
    if (keep) a.out_slots[s] = o;
  }
  a.out_flags[s] = keep ? 1u : 0u;
}

}  // namespace esvo
