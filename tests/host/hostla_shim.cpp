// Test shim: exposes the library's host linear algebra (cusmc_amd/csrc/hostla.h, header-only,
// no HIP) to ctypes so that the CPU suite can check it against numpy.
#include "../../cusmc_amd/csrc/hostla.h"

extern "C" void shim_ql_factor(const double *M, int n, double *L, double *Qt)
{
  std::vector<double> l, q;
  cusmc::la::ql_factor(M, n, l, q);
  std::copy(l.begin(), l.end(), L);
  std::copy(q.begin(), q.end(), Qt);
}

// cusmc_dist_create()'s factor (cusmc_abi.hip): W = L^-1 and logdet = sum 2 ln L_jj.  Returns cholesky()'s code.
extern "C" int shim_dist_factor(const double *S, int n, double *W, double *logdet)
{
  std::vector<double> L, w;
  const int rc = cusmc::la::cholesky(S, n, L);
  if (rc) return rc;
  cusmc::la::lower_inverse(L, n, w);
  std::copy(w.begin(), w.end(), W);
  double ld = 0.0;
  for (int i = 0; i < n; ++i) ld += 2.0 * std::log(L[(size_t)i * n + i]);
  *logdet = ld;
  return 0;
}

// plan_affine()'s factor and bias (cusmc_abi.hip) for a general F: M = -W F, QL-rotated when n >= 16 and M is
// not lower triangular; bias = W y, rotated by Q^T with it.  z = bias + M x.
extern "C" void shim_plan_affine(const double *W, const double *F, const double *y, int n, double *M, double *bias)
{
  std::vector<double> m, b, L, Qt;
  cusmc::la::matmul(W, F, n, m);
  for (double &v : m) v = -v;
  if (n >= 16 && !cusmc::la::is_lower_triangular(m.data(), n)) {
    cusmc::la::ql_factor(m.data(), n, L, Qt);
    m.swap(L);
  }
  cusmc::la::matvec(W, y, n, b);
  if (!Qt.empty()) {
    std::vector<double> rb;
    cusmc::la::matvec(Qt.data(), b.data(), n, rb);
    b.swap(rb);
  }
  std::copy(m.begin(), m.end(), M);
  std::copy(b.begin(), b.end(), bias);
}

extern "C" double shim_mvt_log_const(double nu, double nu_plus_d, int d) { return cusmc::la::mvt_log_const(nu, nu_plus_d, d); }
