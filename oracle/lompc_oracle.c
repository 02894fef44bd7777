/*
 * lompc_oracle.c — CPU ORACLE for the LoMPC hot path. TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load
 * this library, and only as the checker / the timed CPU baseline.  The product
 * (incentive-design-mpc_amd/) never links or calls it.
 *
 * Plain-C restatement of oracle/lompc_oracle.py (itself a restatement of the
 * reference AkshayThiru/incentive-design-mpc, chargingstation/lompc.py):
 *   - build_qp      lompc.py:101-135 -> dense H (N x N), g, c0
 *                   (A = tril(ones) lompc.py:69, q_scale lompc.py:67)
 *   - objective     literal cost expression, lompc.py:95-135 / :155
 *   - solve         the unique optimum asked of Clarabel at lompc.py:152,
 *                   computed by a DENSE primal active-set method (Cholesky of
 *                   the free block every iteration), PWL kinks as knots.
 *   - batch         the per-EV loop of price_solver.py:203-209, optionally
 *                   spread over OpenMP threads (the reference loop is serial).
 * Same algorithm and tolerances as the Python oracle; cross-checked against it
 * and against the 50-digit golden vectors in tests/.
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define OMAXN 128
/* margin of the release test over one coordinate's forward error bound (lompc_oracle.py) */
#define RELEASE_ULPS 8.0

typedef struct {
  int N, small;
  double delta, theta, y_max, w_max, q_scale;
  double knots[5], slopes[4];
  int m;
} ocfg;

static void cfg_init(ocfg* c, int N, int small, double delta, double theta, double y_max, double w_max) {
  c->N = N;
  c->small = small;
  c->delta = delta;
  c->theta = theta;
  c->y_max = y_max;
  c->w_max = w_max;
  c->q_scale = 3 * theta / (4 * w_max); /* lompc.py:67 */
  if (small) {
    c->m = 1;
    c->knots[0] = 0.0;
    c->knots[1] = w_max;
    c->slopes[0] = 0.0;
  } else { /* lompc.py:108-114 */
    static const double kr[5] = {0.0, 0.125, 0.5, 0.75, 1.0};
    static const double sr[4] = {0.0, 1.0, 1.5, 2.0};
    double sc = (theta * w_max) * (theta * w_max) / w_max;
    c->m = 4;
    for (int k = 0; k < 5; ++k) c->knots[k] = w_max * kr[k];
    for (int k = 0; k < 4; ++k) c->slopes[k] = sc * sr[k];
  }
}

/* H = 2 delta theta^2 A'A + 2 lmbd_r theta^2 I + 2 q_scale diag(l3) [+ 2 theta^2/0.81 I]
 * g = theta (l1 - l2) - 2 delta theta^2 gamma A'1 ;  c0 = theta w_max sum(l2) */
static void build_qp(const ocfg* c, const double* lmbd, double lmbd_r, double gamma, double* H, double* g,
                     double* c0) {
  const int N = c->N;
  const double th = c->theta, de = c->delta;
  double s2 = 0.0;
  for (int j = 0; j < N; ++j) {
    for (int k = 0; k < N; ++k) {
      int mx = j > k ? j : k;
      H[j * N + k] = 2 * de * th * th * (double)(N - mx);
    }
    H[j * N + j] += 2 * lmbd_r * th * th + 2 * c->q_scale * lmbd[2 * N + j];
    if (c->small) H[j * N + j] += 2 * th * th / (0.9 * 0.9);
    g[j] = th * (lmbd[j] - lmbd[N + j]) - 2 * de * th * th * gamma * (double)(N - j);
    s2 += lmbd[N + j];
  }
  *c0 = th * c->w_max * s2;
}

/* literal objective, lompc.py:95-135 */
static double objective(const ocfg* c, const double* w, const double* lmbd, double lmbd_r, double gamma) {
  const int N = c->N;
  const double th = c->theta;
  double cost = 0.0, y = 0.0, syy = 0.0, sy = 0.0, lp = 0.0, qp = 0.0, rp = 0.0;
  if (c->small) {
    for (int j = 0; j < N; ++j) cost += th * th * (w[j] / 0.9) * (w[j] / 0.9);
  } else {
    double pwl = 0.0;
    for (int j = 0; j < N; ++j) {
      double u = w[j] / c->w_max;
      double v = 0.0 * u;
      if (u - 0.125 > v) v = u - 0.125;
      if (1.5 * u - 0.375 > v) v = 1.5 * u - 0.375;
      if (2 * u - 0.75 > v) v = 2 * u - 0.75;
      pwl += v;
    }
    cost += (th * c->w_max) * (th * c->w_max) * pwl;
  }
  for (int j = 0; j < N; ++j) {
    y += w[j];
    syy += y * y;
    sy += y;
    lp += lmbd[j] * w[j] + lmbd[N + j] * (c->w_max - w[j]);
    qp += lmbd[2 * N + j] * w[j] * w[j];
    rp += w[j] * w[j];
  }
  cost += c->delta * th * th * (syy - 2 * gamma * sy);
  cost += th * lp + c->q_scale * qp + lmbd_r * th * th * rp;
  return cost;
}

/* in-place Cholesky solve of the n x n SPD matrix M (row-major), rhs b -> x */
static int chol_solve(int n, double* M, double* b) {
  for (int j = 0; j < n; ++j) {
    double s = M[j * n + j];
    for (int k = 0; k < j; ++k) s -= M[j * n + k] * M[j * n + k];
    if (!(s > 0.0)) return -1;
    double d = sqrt(s);
    M[j * n + j] = d;
    for (int i = j + 1; i < n; ++i) {
      double t = M[i * n + j];
      for (int k = 0; k < j; ++k) t -= M[i * n + k] * M[j * n + k];
      M[i * n + j] = t / d;
    }
  }
  for (int i = 0; i < n; ++i) {
    double t = b[i];
    for (int k = 0; k < i; ++k) t -= M[i * n + k] * b[k];
    b[i] = t / M[i * n + i];
  }
  for (int i = n - 1; i >= 0; --i) {
    double t = b[i];
    for (int k = i + 1; k < n; ++k) t -= M[k * n + i] * b[k];
    b[i] = t / M[i * n + i];
  }
  return 0;
}

/* Dense primal active set (Nocedal & Wright Alg. 16.3), as oracle/lompc_oracle.py */
/* warm != 0: start from the working set already in st (a feasible point: fixed coordinates at
 * their knot, free ones at their segment's midpoint) instead of w = 0 with every coordinate at 0 */
static int solve_one(const ocfg* c, const double* H, const double* g, double* w, int* st, int* iters, int warm) {
  const int N = c->N;
  double wh[OMAXN], p[OMAXN], rhs[OMAXN], M[OMAXN * OMAXN];
  int F[OMAXN];
  /* release / termination tolerance, per coordinate: RELEASE_ULPS (N + 2) eps times the magnitudes
   * that enter (Hw + g)_j + slope (lompc_oracle.py solve_state); nothing of the other coordinates */
  const double noise = RELEASE_ULPS * (double)(N + 2) * DBL_EPSILON;
  for (int j = 0; j < N; ++j) {
    if (!warm) st[j] = 0;
    w[j] = (st[j] & 1) ? 0.5 * (c->knots[(st[j] - 1) >> 1] + c->knots[(st[j] + 1) >> 1]) : c->knots[st[j] >> 1];
  }
  for (int it = 0; it < 100000; ++it) {
    int nf = 0;
    for (int j = 0; j < N; ++j) {
      if (st[j] & 1) F[nf++] = j;
      else wh[j] = c->knots[st[j] >> 1];
    }
    for (int a = 0; a < nf; ++a) {
      int j = F[a];
      double s = g[j] + c->slopes[(st[j] - 1) >> 1];
      for (int k = 0; k < N; ++k)
        if (!(st[k] & 1)) s += H[j * N + k] * wh[k];
      rhs[a] = -s;
      for (int b = 0; b < nf; ++b) M[a * nf + b] = H[j * N + F[b]];
    }
    if (nf && chol_solve(nf, M, rhs)) return -2;
    for (int a = 0; a < nf; ++a) wh[F[a]] = rhs[a];
    double alpha = 1.0;
    int blk = -1, bk = 0;
    for (int j = 0; j < N; ++j) {
      p[j] = wh[j] - w[j];
      if (!(st[j] & 1)) continue;
      int k = (st[j] - 1) >> 1;
      double a;
      if (p[j] > 0) {
        a = (c->knots[k + 1] - w[j]) / p[j];
        if (a < alpha) { alpha = a; blk = j; bk = k + 1; }
      } else if (p[j] < 0) {
        a = (c->knots[k] - w[j]) / p[j];
        if (a < alpha) { alpha = a; blk = j; bk = k; }
      }
    }
    if (blk < 0) {
      memcpy(w, wh, N * sizeof(double));
      double best = 0.0;
      int bj = -1, bd = 0;
      for (int j = 0; j < N; ++j) {
        if (st[j] & 1) continue;
        double r = g[j], mag = fabs(g[j]);
        for (int k = 0; k < N; ++k) {
          r += H[j * N + k] * w[k];
          mag += fabs(H[j * N + k]) * fabs(w[k]);
        }
        int k = st[j] >> 1;
        if (k < c->m) {
          double v = -r - c->slopes[k];
          if (v > best && v > noise * (mag + fabs(c->slopes[k]))) { best = v; bj = j; bd = 1; }
        }
        if (k > 0) {
          double v = r + c->slopes[k - 1];
          if (v > best && v > noise * (mag + fabs(c->slopes[k - 1]))) { best = v; bj = j; bd = -1; }
        }
      }
      if (bj < 0) {
        if (iters) *iters = it + 1;
        return 0;
      }
      st[bj] += bd;
    } else {
      if (alpha < 0) alpha = 0;
      for (int j = 0; j < N; ++j) w[j] += alpha * p[j];
      st[blk] = 2 * bk;
      w[blk] = c->knots[bk];
    }
  }
  return -1;
}

int oracle_abi_version(void) { return 1; }

/* One QP: returns 0 on success. */
int oracle_lompc_solve(int N, int ev_small, double delta, double theta, double y_max, double w_max,
                       const double* lmbd, double lmbd_r, double gamma, double* w, double* cost, int* iters) {
  if (N < 1 || N > OMAXN) return -3;
  ocfg c;
  cfg_init(&c, N, ev_small, delta, theta, y_max, w_max);
  double* H = (double*)malloc((size_t)N * N * sizeof(double));
  double g[OMAXN], c0;
  int st[OMAXN];
  build_qp(&c, lmbd, lmbd_r, gamma, H, g, &c0);
  int rc = solve_one(&c, H, g, w, st, iters, 0);
  if (cost) *cost = objective(&c, w, lmbd, lmbd_r, gamma);
  free(H);
  return rc;
}

/* Batch of B QPs sharing lmbd / lmbd_r (one parameter set), per-EV gamma.
 * nthreads <= 0: OpenMP default. Returns the number of failed solves. */
int64_t oracle_lompc_solve_batch(int N, int ev_small, double delta, double theta, double y_max, double w_max,
                                 const double* lmbd, double lmbd_r, int64_t B, const double* gamma, double* w,
                                 double* cost, int nthreads) {
  if (N < 1 || N > OMAXN) return -1;
  int64_t nfail = 0;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel reduction(+ : nfail)
#endif
  {
    ocfg c;
    cfg_init(&c, N, ev_small, delta, theta, y_max, w_max);
    double* H = (double*)malloc((size_t)N * N * sizeof(double));
    double g[OMAXN], c0;
    int st[OMAXN];
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 16)
#endif
    for (int64_t i = 0; i < B; ++i) {
      build_qp(&c, lmbd, lmbd_r, gamma[i], H, g, &c0);
      int rc = solve_one(&c, H, g, w + i * N, st, NULL, 0);
      if (rc) nfail += 1;
      if (cost) cost[i] = objective(&c, w + i * N, lmbd, lmbd_r, gamma[i]);
    }
    free(H);
  }
  return nfail;
}

/* As oracle_lompc_solve_batch, but each thread walks a contiguous range of the batch and starts
 * every solve from the working set its previous solve ended with (the same dense active set and
 * the same final equality-constrained solve: only the start differs).  With gamma sorted, nearby
 * EVs share most of their optimal working set, so a solve takes a few iterations instead of
 * O(N): the test checker for config-5-sized partitions (tests/test_gpu_price_loop_c5.py). */
int64_t oracle_lompc_solve_batch_warm(int N, int ev_small, double delta, double theta, double y_max, double w_max,
                                      const double* lmbd, double lmbd_r, int64_t B, const double* gamma, double* w,
                                      double* cost, int nthreads) {
  if (N < 1 || N > OMAXN) return -1;
  int64_t nfail = 0;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel reduction(+ : nfail)
#endif
  {
    ocfg c;
    cfg_init(&c, N, ev_small, delta, theta, y_max, w_max);
    double* H = (double*)malloc((size_t)N * N * sizeof(double));
    double g[OMAXN], c0;
    int st[OMAXN];
    int warm = 0;
#ifdef _OPENMP
#pragma omp for schedule(static)
#endif
    for (int64_t i = 0; i < B; ++i) {
      build_qp(&c, lmbd, lmbd_r, gamma[i], H, g, &c0);
      int rc = solve_one(&c, H, g, w + i * N, st, NULL, warm);
      if (rc) { /* a warm start that failed: once more from w = 0 */
        rc = solve_one(&c, H, g, w + i * N, st, NULL, 0);
      }
      warm = rc == 0;
      if (rc) nfail += 1;
      if (cost) cost[i] = objective(&c, w + i * N, lmbd, lmbd_r, gamma[i]);
    }
    free(H);
  }
  return nfail;
}

/* As oracle_lompc_solve_batch, but every EV keeps its own working set between calls (state, B x N
 * bytes, caller-owned; *fresh != 0: no stored sets yet, every solve starts cold and *fresh is
 * cleared).  A price loop's consecutive iterations move the prices a little, so most EVs end on the
 * working set they ended on before: one equality-constrained solve and the optimality check.  The
 * same dense active set and termination test as every other entry (only the start differs). */
int64_t oracle_lompc_solve_batch_state(int N, int ev_small, double delta, double theta, double y_max, double w_max,
                                       const double* lmbd, double lmbd_r, int64_t B, const double* gamma, double* w,
                                       double* cost, unsigned char* state, int* fresh, int nthreads) {
  if (N < 1 || N > OMAXN) return -1;
  int64_t nfail = 0;
  const int warm0 = !*fresh;
#ifdef _OPENMP
  if (nthreads > 0) omp_set_num_threads(nthreads);
#pragma omp parallel reduction(+ : nfail)
#endif
  {
    ocfg c;
    cfg_init(&c, N, ev_small, delta, theta, y_max, w_max);
    double* H = (double*)malloc((size_t)N * N * sizeof(double));
    double g[OMAXN], c0;
    int st[OMAXN];
#ifdef _OPENMP
#pragma omp for schedule(dynamic, 64)
#endif
    for (int64_t i = 0; i < B; ++i) {
      unsigned char* s = state + i * N;
      for (int j = 0; j < N; ++j) st[j] = warm0 ? s[j] : 0;
      build_qp(&c, lmbd, lmbd_r, gamma[i], H, g, &c0);
      int rc = solve_one(&c, H, g, w + i * N, st, NULL, warm0);
      if (rc && warm0) rc = solve_one(&c, H, g, w + i * N, st, NULL, 0);
      if (rc) nfail += 1;
      for (int j = 0; j < N; ++j) s[j] = (unsigned char)st[j];
      if (cost) cost[i] = objective(&c, w + i * N, lmbd, lmbd_r, gamma[i]);
    }
    free(H);
  }
  *fresh = 0;
  return nfail;
}

int oracle_max_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}
