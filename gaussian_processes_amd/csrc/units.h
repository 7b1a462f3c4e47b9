// The vocabulary of the entry points that run several units in one call (the single call is the group of one): the
// units of a call and "member X of every unit's context" (Units), a context's work matrices as a chain of the
// lock-step factorisation (add_k_chain, add_v_chain), and the refusals every such call shares (Refuse, unit_prefix,
// unit_context_refusal).  A new group entry point is built from these.  Internal header; host only, nothing here
// allocates.
#pragma once
#include "product.h"
#include <string>

namespace gpfit {

// The units of a call, or of one launch of it (the admitted ones; those that still have a step): each with its context
// and its index in the caller's tables, in ascending order.  Whatever a body keeps per unit beside the contexts -- the
// caller's operands, what the admission found -- is indexed like the caller's tables, and table() / mats(ld, f) hand
// that index to f; a launch's tables and lists are in the order of the list.
struct Units {
  int cnt = 0;
  gpfit_ctx* ctx[CHAIN_MAXU];
  int at[CHAIN_MAXU];
  void add(gpfit_ctx* c, int u) { ctx[cnt] = c; at[cnt++] = u; }
  static Units all(gpfit_ctx* const* ctxs, int n) {
    Units l;
    for (int u = 0; u < n && u < CHAIN_MAXU; ++u) l.add(ctxs[u], u);
    return l;
  }
  // one chain of a lock-step batch per unit: all of them
  uint32_t chains() const { return (uint32_t)((1ull << cnt) - 1ull); }

  template <typename T, typename F>
  PerUnit<T> table(F&& f) const {
    PerUnit<T> t{};
    for (int i = 0; i < cnt; ++i) t.v[i] = f(at[i]);
    return t;
  }
  template <typename T>
  PerUnit<T> same(T v) const { return table<T>([&](int) { return v; }); }
  // the units' entries of a table indexed like the caller's
  template <typename T>
  PerUnit<T> from(const T* tab) const { return table<T>([&](int u) { return tab[u]; }); }
  // member X of every unit's context (off elements into it); cof: to read only
  template <typename T>
  PerUnit<T*> of(T* gpfit_ctx::*X, int64_t off = 0) const {
    PerUnit<T*> t{};
    for (int i = 0; i < cnt; ++i) t.v[i] = ctx[i]->*X + off;
    return t;
  }
  PerUnit<const double*> cof(double* gpfit_ctx::*X) const {
    PerUnit<const double*> t{};
    for (int i = 0; i < cnt; ++i) t.v[i] = ctx[i]->*X;
    return t;
  }
  PerUnit<double*> scal(int slot) const { return of(&gpfit_ctx::scal, slot); }
  // work matrix X of every unit's context as the operand of one product: the block at (row, col), leading dimension ld
  Mat<double> mats(double* gpfit_ctx::*X, int64_t ld, int row = 0, int col = 0) const {
    return gpfit::mats(cnt, ld, [&](int i) { return ctx[i]->*X + (int64_t)row * ld + col; });
  }
  // the same for a table of pointers indexed like the caller's: each unit's matrix as it stands
  template <typename P>
  Mat<P> mats(P* const* tab, int64_t ld) const {
    return gpfit::mats(cnt, ld, [&](int i) { return tab[at[i]]; });
  }
};

// A context's work matrices as one more chain of a lock-step batch (the workspace is allocated for fp64; R = float
// reads it as fp32); returns the chain's index.  K~'s chain: Kbuf, Lbuf, Libuf, Tmp, reporting into info word INFO_K;
// V's chain: Vbuf, LVbuf, LiVbuf, TmpV, into INFO_V unless the caller factors something else there.
template <typename R>
int add_chain(CholBatchT<R>& cb, double* A, double* L, double* Li, double* Tmp, int* info) {
  const int b = cb.nb++;
  cb.A[b] = reinterpret_cast<R*>(A); cb.L[b] = reinterpret_cast<R*>(L); cb.Li[b] = reinterpret_cast<R*>(Li);
  cb.Tmp[b] = reinterpret_cast<R*>(Tmp); cb.info[b] = info;
  return b;
}
template <typename R>
int add_k_chain(CholBatchT<R>& cb, gpfit_ctx* c) {
  return add_chain(cb, c->Kbuf, c->Lbuf, c->Libuf, c->Tmp, c->info + INFO_K);
}
template <typename R>
int add_v_chain(CholBatchT<R>& cb, gpfit_ctx* c, InfoWord word = INFO_V) {
  return add_chain(cb, c->Vbuf, c->LVbuf, c->LiVbuf, c->TmpV, c->info + word);
}

// "<entry point>: <why>" as the error string; -3
struct Refuse {
  const char* name;
  int operator()(const std::string& why) const {
    set_error(std::string(name) + ": " + why);
    return -3;
  }
};
// what a refusal that concerns one unit of several begins with (the single call names no unit)
inline std::string unit_prefix(int n_units, int u) { return n_units > 1 ? "unit " + std::to_string(u) + ": " : std::string(); }

// What a call of several units asks of unit u's context, given those before it: nullptr, or the sentence of the
// refusal.  pending: the sentence of a body that words the last one differently.
inline const char* unit_context_refusal(gpfit_ctx* const* ctxs, int u, const char* pending = GP_PENDING_REFUSAL) {
  if (ctxs[u]->device != ctxs[0]->device) return "the contexts of one call must live on one device";
  for (int v = 0; v < u; ++v)
    if (ctxs[v] == ctxs[u]) return "every unit needs a context of its own";
  if (ctxs[u]->pend.active) return pending;
  return nullptr;
}

}  // namespace gpfit
