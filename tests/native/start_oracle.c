/* tests/native/start_oracle.c -- TEST HARNESS ONLY.
 *
 * The oracle's solve of the MPC NLP from a caller's starting point: what the reference computes
 * when a point is passed as CppAD::ipopt::solve's xi.  A shim built by tests/test_start_host.py
 * against oracle/_build/liboracle.so: MPC::Solve's bounds from ora_mpc_bounds, the public
 * ora_mpc_fg / _grad_f / _jac_g / _hess as the NLP's callbacks, the caller's x0 in place of
 * MPC::Solve's, then ora_ipm_solve (which scales at x0 and pushes it inside the bounds).
 */
#include <stdlib.h>
#include <string.h>

#include "ora.h"

typedef struct {
    const ora_mpc_params* p;
    const double* c;
    double* fg;
} so_ctx;

static double so_f(void* ctx, const double* x) {
    so_ctx* m = (so_ctx*)ctx;
    ora_mpc_fg(m->p, m->c, x, m->fg);
    return m->fg[0];
}
static void so_grad(void* ctx, const double* x, double* g) {
    so_ctx* m = (so_ctx*)ctx;
    ora_mpc_grad_f(m->p, m->c, x, g);
}
static void so_g(void* ctx, const double* x, double* g) {
    so_ctx* m = (so_ctx*)ctx;
    ora_mpc_fg(m->p, m->c, x, m->fg);
    memcpy(g, m->fg + 1, sizeof(double) * (size_t)ora_mpc_ng(m->p->steps));
}
static void so_jac(void* ctx, const double* x, double* J) {
    so_ctx* m = (so_ctx*)ctx;
    ora_mpc_jac_g(m->p, m->c, x, J);
}
static void so_hess(void* ctx, const double* x, double sigma, const double* lam, double* H) {
    so_ctx* m = (so_ctx*)ctx;
    ora_mpc_hess(m->p, m->c, x, sigma, lam, H);
}

/* x0[nx]: the starting point; x[nx] out; returns the status, *iters the iteration count */
int start_oracle_solve(const ora_mpc_params* p, const ora_ipm_opts* opts, const double* state6,
                       const double* coeffs4, const double* x0, double* x, int* iters) {
    const int N = p->steps, nx = ora_mpc_nx(N), ng = ora_mpc_ng(N);
    double* buf = (double*)malloc(sizeof(double) * (size_t)(5 * nx + 5 * ng + 1));
    double *d0 = buf, *xl = d0 + nx, *xu = xl + nx, *zl = xu + nx, *zu = zl + nx;
    double *gl = zu + nx, *gu = gl + ng, *lam = gu + ng, *gv = lam + ng, *fg = gv + ng;
    ora_mpc_bounds(p, state6, d0, xl, xu, gl, gu); /* (d0: MPC::Solve's own start, not used) */
    so_ctx ctx = {p, coeffs4, fg};
    ora_nlp nlp;
    memset(&nlp, 0, sizeof nlp);
    nlp.n = nx;
    nlp.m = ng;
    nlp.ctx = &ctx;
    nlp.f = so_f;
    nlp.grad_f = so_grad;
    nlp.g = so_g;
    nlp.jac_g = so_jac;
    nlp.hess = so_hess;
    nlp.xl = xl;
    nlp.xu = xu;
    nlp.gl = gl;
    nlp.gu = gu;
    nlp.x0 = x0;
    /* the KKT rows stage by stage (ora_ipm_opts.kkt_structured): the rows into stage k, its
     * state, its control */
    int* kord = (int*)malloc(sizeof(int) * (size_t)(nx + ng));
    int q = 0;
    for (int k = 0; k < N; ++k) {
        for (int s = 0; s < 6; ++s) kord[q++] = nx + s * N + k;
        for (int s = 0; s < 6; ++s) kord[q++] = s * N + k;
        if (k < N - 1) {
            kord[q++] = 6 * N + k;
            kord[q++] = 7 * N - 1 + k;
        }
    }
    nlp.kkt_order = kord;
    ora_ipm_result res;
    const int status = ora_ipm_solve(&nlp, opts, x, zl, zu, lam, gv, &res);
    if (iters) *iters = res.iters;
    free(kord);
    free(buf);
    return status;
}
