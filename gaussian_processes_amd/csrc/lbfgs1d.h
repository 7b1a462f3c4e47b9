// L-BFGS with the strong-Wolfe line search for one scalar parameter: a port of torch/optim/lbfgs.py
// (torch 2.10: LBFGS.step with line_search_fn='strong_wolfe', _strong_wolfe, _cubic_interpolate),
// operation by operation in fp64, for the host and for the device.  Internal header.
//
// What makes it the same computation as torch's on a one-element parameter:
//  - every scalar operation rounds on its own (contraction is off in every function here), as
//    torch's scalar tensor ops and Python floats do;
//  - the three `add_(..., alpha=a)` of torch (the parameter update x + t d and the two loops of the
//    two-loop recursion) are one fused multiply-add: ATen's CPU add kernel computes self + alpha * other
//    as a fused operation (tests/test_fparam_lbfgs_cpu.py checks that property of the installed torch);
//  - Python's builtin min / max keep their first argument unless the second compares less / greater,
//    which fixes where NaN goes;
//  - a Python float divided by a tensor is the tensor's reciprocal times the float (Tensor.__rtruediv__),
//    two roundings instead of one.  The only such division is 3 (f1 - f2) / (x1 - x2) of the cubic
//    interpolation when a step there is a tensor, so every step carries whether torch holds it as a tensor
//    (the first step min(1, 1/|g|) lr when 1/|g| < 1, every interpolation result, and what is computed from them);
//  - every loop is bounded by torch's own counters (n_iter < max_iter, ls_iter < max_ls), so a NaN
//    comparison cannot make one unbounded.
//
// The objective is a callable  bool obj(double x, double* loss, double* grad):  false stands for a
// closure that raised, and stops the optimiser with status = the 1-based number of that call.
// The history pairs (y, s, 1/ys) and the two-loop coefficients live in caller storage of
// history_size doubles each, kept as a ring in the order of torch's lists; the Slots policy writes
// them (on the device: one thread writes, a barrier publishes).
#pragma once
#include <cfloat>
#include <cmath>

#if defined(__HIPCC__)
#define GP_LB_HD __host__ __device__
#else
#define GP_LB_HD
#endif

namespace gpfit {

struct Lbfgs1dConfig {
  double lr = 1.0, tolerance_grad = 1e-7, tolerance_change = 1e-9;
  int max_iter = 20, max_eval = 25, history_size = 100;
};

struct Lbfgs1dResult {
  double x = 0.0;           // final parameter
  double first_loss = 0.0;  // the loss step() returns (its first closure call)
  double last_loss = 0.0;   // the loss at the final parameter as the optimiser holds it
  int n_evals = 0;          // closure calls
  int n_iter = 0;           // iterations (torch's state["n_iter"] of a fresh optimiser)
  int status = 0;           // 0, or the 1-based number of the closure call that failed
};

struct Lbfgs1dStorage {
  double *y, *s, *ro, *al;  // [history_size] each
};

// math.isfinite (the same test on host and device)
GP_LB_HD inline bool lbfgs1d_finite(double v) { return fabs(v) <= DBL_MAX; }

// Python's builtin max(a, b) and min(a, b)
GP_LB_HD inline double py_max(double a, double b) { return (b > a) ? b : a; }
GP_LB_HD inline double py_min(double a, double b) { return (b < a) ? b : a; }

// _cubic_interpolate (lbfgs.py:12-37); bounds given when has_bounds.  x1t, x2t, bmint, bmaxt: whether torch holds
// those steps as tensors; rt receives that for the result.
GP_LB_HD inline double lbfgs1d_cubic(double x1, bool x1t, double f1, double g1, double x2, bool x2t, double f2,
                                     double g2, bool has_bounds, double bmin, bool bmint, double bmax, bool bmaxt,
                                     bool& rt) {
#pragma clang fp contract(off)
  double xmin_bound, xmax_bound;
  bool xmin_t, xmax_t;
  if (has_bounds) {
    xmin_bound = bmin; xmin_t = bmint;
    xmax_bound = bmax; xmax_t = bmaxt;
  } else if (x1 <= x2) {
    xmin_bound = x1; xmin_t = x1t;
    xmax_bound = x2; xmax_t = x2t;
  } else {
    xmin_bound = x2; xmin_t = x2t;
    xmax_bound = x1; xmax_t = x1t;
  }
  const double num = 3.0 * (f1 - f2), den = x1 - x2;  // losses are Python floats
  const double d1 = g1 + g2 - ((x1t || x2t) ? (1.0 / den) * num : num / den);
  const double d2_square = d1 * d1 - g1 * g2;  // d1**2 of a tensor is d1 * d1 in ATen
  if (d2_square >= 0) {
    const double d2 = sqrt(d2_square);
    double min_pos;
    if (x1 <= x2)
      min_pos = x2 - (x2 - x1) * ((g2 + d2 - d1) / (g2 - g1 + 2.0 * d2));
    else
      min_pos = x1 - (x1 - x2) * ((g1 + d2 - d1) / (g1 - g2 + 2.0 * d2));
    // min(max(min_pos, xmin_bound), xmax_bound), min_pos being a tensor
    const bool lo = xmin_bound > min_pos;
    const double v = lo ? xmin_bound : min_pos;
    const bool vt = lo ? xmin_t : true;
    const bool hi = xmax_bound < v;
    rt = hi ? xmax_t : vt;
    return hi ? xmax_bound : v;
  }
  rt = xmin_t || xmax_t;
  return (xmin_bound + xmax_bound) / 2.0;
}

// One closure call at x + t d (_directional_evaluate; the parameter is x + t d with one rounding)
template <class Obj>
GP_LB_HD inline bool lbfgs1d_eval(Obj& obj, double x, double t, double d, double* f, double* g, int& n_evals) {
  ++n_evals;
  return obj(fma(t, d, x), f, g);
}

// A point of the line search: step, loss, gradient, directional derivative, and whether torch holds the step as a
// tensor
struct Lbfgs1dPoint {
  double t, f, g, gtd;
  bool tt;
};

// _strong_wolfe (lbfgs.py:40-200) with c1 = 1e-4, c2 = 0.9.  On return t, f, g are the bracket's low
// point; false when a closure call failed.  The bracket's two positions are named variables (b0, b1), not an
// array indexed at run time, so that they stay in registers.
template <class Obj>
GP_LB_HD inline bool lbfgs1d_strong_wolfe(Obj& obj, double x, double& t, bool t_tensor, double d, double& f, double& g,
                                          double gtd, double tolerance_change, int max_ls, int& ls_func_evals,
                                          int& n_evals) {
#pragma clang fp contract(off)
  const double c1 = 1e-4, c2 = 0.9;
  const double d_norm = fabs(d);
  Lbfgs1dPoint nw{t, 0.0, 0.0, 0.0, t_tensor};  // f_new, g_new, gtd_new at t
  Lbfgs1dPoint prev{0.0, f, g, gtd, false};     // t_prev (the int 0), f_prev, g_prev, gtd_prev
  bool done = false;
  int ls_iter = 0;
  bool one_point = false;  // the bracket is [t] (first phase ended on the Wolfe conditions)
  Lbfgs1dPoint b0{0.0, 0.0, 0.0, 0.0, false}, b1{0.0, 0.0, 0.0, 0.0, false};
  // torch evaluates at the initial step and then at the end of every bracketing iteration; here the evaluation heads
  // the loop (one call site: every inlined copy of the objective costs registers on the device)
  for (bool first = true;; first = false) {
    nw.t = t;
    nw.tt = t_tensor;
    if (!lbfgs1d_eval(obj, x, t, d, &nw.f, &nw.g, n_evals)) return false;
    nw.gtd = nw.g * d;
    if (first) {
      ls_func_evals = 1;
    } else {
      ls_func_evals += 1;
      ls_iter += 1;
    }
    if (!(ls_iter < max_ls)) break;
    if (nw.f > (f + c1 * t * gtd) || (ls_iter > 1 && nw.f >= prev.f)) {
      b0 = prev;
      b1 = nw;
      break;
    }
    if (fabs(nw.gtd) <= -c2 * gtd) {
      one_point = true;
      b0 = nw;
      done = true;
      break;
    }
    if (nw.gtd >= 0) {
      b0 = prev;
      b1 = nw;
      break;
    }
    // interpolate
    const double min_step = t + 0.01 * (t - prev.t);
    const double max_step = t * 10.0;
    t = lbfgs1d_cubic(prev.t, prev.tt, prev.f, prev.gtd, nw.t, nw.tt, nw.f, nw.gtd, true, min_step, nw.tt || prev.tt,
                      max_step, nw.tt, t_tensor);
    prev = nw;
  }
  // reached max number of iterations?  (the breaks above only happen with ls_iter < max_ls; bracket_gtd is not
  // assigned here, and the zoom below does not run)
  if (ls_iter == max_ls) {
    b0 = Lbfgs1dPoint{0.0, f, g, b0.gtd, false};
    b1 = Lbfgs1dPoint{t, nw.f, nw.g, b1.gtd, t_tensor};
  }

  // zoom phase
  bool insuf_progress = false;
  // low_pos, high_pos = (0, 1) if bracket_f[0] <= bracket_f[-1] else (1, 0).  With a one-point bracket a NaN loss
  // would make torch index past it (IndexError); the point itself is returned here.
  bool low1 = one_point ? false : !(b0.f <= b1.f);  // low_pos == 1
  while (!done && ls_iter < max_ls) {
    if (fabs(b1.t - b0.t) * d_norm < tolerance_change) break;
    t = lbfgs1d_cubic(b0.t, b0.tt, b0.f, b0.gtd, b1.t, b1.tt, b1.f, b1.gtd, false, 0.0, false, 0.0, false, t_tensor);
    // max(bracket), min(bracket): the first entry unless the second compares greater / less
    const bool max1 = b1.t > b0.t, min1 = b1.t < b0.t;
    const double bmax = max1 ? b1.t : b0.t, bmin = min1 ? b1.t : b0.t;
    const bool bmax_t = max1 ? b1.tt : b0.tt, bmin_t = min1 ? b1.tt : b0.tt;
    const double eps = 0.1 * (bmax - bmin);
    const bool eps_t = bmax_t || bmin_t;
    if (py_min(bmax - t, t - bmin) < eps) {
      if (insuf_progress || t >= bmax || t <= bmin) {
        if (fabs(t - bmax) < fabs(t - bmin)) {
          t = bmax - eps;
          t_tensor = bmax_t || eps_t;
        } else {
          t = bmin + eps;
          t_tensor = bmin_t || eps_t;
        }
        insuf_progress = false;
      } else {
        insuf_progress = true;
      }
    } else {
      insuf_progress = false;
    }
    nw.t = t;
    nw.tt = t_tensor;
    if (!lbfgs1d_eval(obj, x, t, d, &nw.f, &nw.g, n_evals)) return false;
    ls_func_evals += 1;
    nw.gtd = nw.g * d;
    ls_iter += 1;

    const Lbfgs1dPoint lo = low1 ? b1 : b0;
    if (nw.f > (f + c1 * t * gtd) || nw.f >= lo.f) {
      // Armijo condition not satisfied or not lower than lowest point: the new point replaces the high one
      if (low1)
        b0 = nw;
      else
        b1 = nw;
      low1 = !(b0.f <= b1.f);
    } else {
      if (fabs(nw.gtd) <= -c2 * gtd) {
        done = true;
      } else if (nw.gtd * ((low1 ? b0.t : b1.t) - lo.t) >= 0) {
        // old high becomes new low
        if (low1)
          b0 = lo;
        else
          b1 = lo;
      }
      // new point becomes new low
      if (low1)
        b1 = nw;
      else
        b0 = nw;
    }
  }
  const Lbfgs1dPoint lo = low1 ? b1 : b0;
  t = lo.t;
  f = lo.f;
  g = lo.g;
  return true;
}

// LBFGS(lr, max_iter, max_eval, tolerance_grad, tolerance_change, history_size,
// line_search_fn='strong_wolfe').step(closure) of a freshly constructed optimiser (lbfgs.py:349-535), from x0.
template <class Slots, class Obj>
GP_LB_HD inline Lbfgs1dResult lbfgs1d_step(Obj& obj, double x0, const Lbfgs1dConfig& cfg, Lbfgs1dStorage h) {
#pragma clang fp contract(off)
  Lbfgs1dResult res;
  double x = x0;
  res.x = x;
  const double lr = cfg.lr, tolerance_grad = cfg.tolerance_grad, tolerance_change = cfg.tolerance_change;
  const int max_iter = cfg.max_iter, max_eval = cfg.max_eval, history_size = cfg.history_size;

  // evaluate initial f(x) and df/dx
  double loss, flat_grad;
  ++res.n_evals;
  if (!obj(x, &loss, &flat_grad)) {
    res.status = res.n_evals;
    return res;
  }
  res.first_loss = loss;
  res.last_loss = loss;
  int current_evals = 1;
  bool opt_cond = fabs(flat_grad) <= tolerance_grad;
  if (opt_cond) return res;

  double d = 0.0, t = 0.0, H_diag = 1.0, prev_flat_grad = 0.0, prev_loss = 0.0;
  int head = 0, num_old = 0;  // ring of the history lists: entry i of torch's lists is slot (head + i) % history_size
  int n_iter = 0;
  while (n_iter < max_iter) {
    n_iter += 1;
    res.n_iter = n_iter;
    // compute gradient descent direction
    if (n_iter == 1) {
      d = -flat_grad;
      H_diag = 1.0;
    } else {
      const double y = flat_grad - prev_flat_grad;
      const double s = d * t;
      const double ys = y * s;
      if (ys > 1e-10) {
        int slot;
        if (num_old == history_size) {  // shift history by one
          slot = head;
          head = (head + 1 == history_size) ? 0 : head + 1;
        } else {
          slot = head + num_old;
          if (slot >= history_size) slot -= history_size;
          num_old += 1;
        }
        Slots::put(h.y, slot, y);
        Slots::put(h.s, slot, s);
        Slots::put(h.ro, slot, 1.0 / ys);
        Slots::publish();
        H_diag = ys / (y * y);
      }
      // two-loop recursion, one buffer
      double q = -flat_grad;
#pragma unroll 1  // rolled: an unrolled copy costs the device kernel registers it does not have at 1024 threads
      for (int i = num_old - 1; i >= 0; --i) {
        int k = head + i;
        if (k >= history_size) k -= history_size;
        const double al = h.s[k] * q * h.ro[k];
        Slots::put(h.al, k, al);
        q = fma(-al, h.y[k], q);
      }
      Slots::publish();
      double r = q * H_diag;
#pragma unroll 1
      for (int i = 0; i < num_old; ++i) {
        int k = head + i;
        if (k >= history_size) k -= history_size;
        const double be_i = h.y[k] * r * h.ro[k];
        r = fma(h.al[k] - be_i, h.s[k], r);
      }
      d = r;
    }
    prev_flat_grad = flat_grad;
    prev_loss = loss;

    // compute step length
    bool t_tensor = false;
    if (n_iter == 1) {
      const double inv = 1.0 / fabs(flat_grad);
      t_tensor = inv < 1.0;  // min(1., 1./flat_grad.abs().sum()) is then the tensor
      t = py_min(1.0, inv) * lr;
    } else {
      t = lr;
    }
    const double gtd = flat_grad * d;
    if (gtd > -tolerance_change) break;

    int ls_func_evals = 0;
    if (!lbfgs1d_strong_wolfe(obj, x, t, t_tensor, d, loss, flat_grad, gtd, tolerance_change,
                              max_eval - current_evals, ls_func_evals, res.n_evals)) {
      res.status = res.n_evals;
      return res;
    }
    x = fma(t, d, x);
    res.x = x;
    res.last_loss = loss;
    opt_cond = fabs(flat_grad) <= tolerance_grad;
    current_evals += ls_func_evals;

    // check conditions
    if (n_iter == max_iter) break;
    if (current_evals >= max_eval) break;
    if (opt_cond) break;
    if (fabs(d * t) <= tolerance_change) break;
    if (fabs(loss - prev_loss) < tolerance_change) break;
  }
  return res;
}

// The closure of varGP's rate-parameter optimiser (utils.py:1490-1500) around one evaluation of the pass.
// Call k evaluates at (logA_k, lambda0_{k-1}) and then sets lambda0_k to the closed form at logA_k; lambda0_0 is the
// closed form at the starting logA, which is where call 1 evaluates: it is taken from that call's pass.  With `fixed`
// every call uses lambda0_fixed instead (f_params carrying loglambda0), while lambda0 is still assigned.  A non-finite
// sum f fails the call, leaving (logA_k, lambda0_k) in fail_x / fail_lambda0.
// Ev: pass(logA) evaluates the totals at A = exp(logA); lambda0_closed() and values(lambda0_used) read them.
struct FparamValues {
  double loglik, dloglik, sum_f;
};

template <class Ev>
struct FparamClosure {
  Ev ev;
  int fixed;
  double lambda0_fixed;
  double lambda0;
  int calls;
  double fail_x, fail_lambda0;
  GP_LB_HD bool operator()(double logA, double* loss, double* grad) {
    ev.pass(logA);
    if (calls++ == 0) lambda0 = ev.lambda0_closed();  // lambda0_given_logA at the start (utils.py:1892)
    const FparamValues v = ev.values(fixed ? lambda0_fixed : lambda0);
    lambda0 = ev.lambda0_closed();
    if (!lbfgs1d_finite(v.sum_f)) {
      fail_x = logA;
      fail_lambda0 = lambda0;
      return false;
    }
    *loss = -v.loglik;
    *grad = -v.dloglik;
    return true;
  }
};

// Slots policy of a single host thread
struct Lbfgs1dHostSlots {
  static void put(double* p, int i, double v) { p[i] = v; }
  static void publish() {}
};

}  // namespace gpfit
