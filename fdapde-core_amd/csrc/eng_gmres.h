// eng_gmres.h -- the restarted GMRES(m) loop of the handles that bring their own operator and buffers (the 2 x 2 block handle, eng_block.hip, and the
// Kronecker-sum handle, eng_kron.hip): the loop of run_gmres (eng_solve.hip) over a vector length n2 -- CGS2 Arnoldi with the k_gm_* kernels, the same stop
// rule (the estimate inside a cycle, the TRUE residual of the preconditioned system at its end, which the next cycle starts from and relres reports).
#ifndef FDAPDE_ENG_GMRES_H
#define FDAPDE_ENG_GMRES_H

#include <algorithm>

#include "context.h"
#include "engine.h"
#include "kernels_block.h"
#include "kernels_gmres.h"

namespace fdapde_engine {

// the handle's buffers: bt = the (preconditioned) right-hand side, x = the iterate on return; r, w, t of n2 words; sc [32], ctl [8]; gm_* sized here
struct HandleGmresWork {
    DBuf<double>&bt, &x, &r, &w, &t, &sc, &gm_V, &gm_s, &gm_part;
    DBuf<int32_t>& ctl;
};

inline int handle_vec_grid(int64_t n2) { return (int)std::max<int64_t>(1, std::min<int64_t>(1024, (n2 + 255) / 256)); }

// op(x, y, stop): y = (the preconditioned operator) x on the context's stream; stop: the device flag every kernel of a cycle reads first, or nullptr
template <class Op> int handle_gmres(fdapde_ctx* c, HandleGmresWork W, int64_t n2, Op&& op, double tol2, int maxit, int32_t h_ctl[4], double h_sc[4]) {
    const int m = c->gmres_m;
    hipStream_t st = c->stream;
    const int vg = handle_vec_grid(n2);
    HIPCHK(c, W.gm_V.alloc((size_t)(m + 1) * (size_t)n2));
    HIPCHK(c, W.gm_s.alloc((size_t)gm_state_doubles(m) + (size_t)m + 2));
    const size_t gm_norm_at = (size_t)(m + 1) * kGmStripes;
    HIPCHK(c, W.gm_part.alloc(gm_norm_at + (size_t)std::max(vg, kGmStripes)));
    double* gm_norm = W.gm_part.p + gm_norm_at;
    double* gs = W.gm_s.p;
    double* h_pass = gs + gm_state_doubles(m);
    double* hcol = gs + 3 * m + 1;
    double* w = W.w.p;
    hipLaunchKernelGGL(k_block_krylov_init, dim3(vg), dim3(256), 0, st, n2, W.bt.p, W.x.p, W.r.p, W.gm_part.p);
    hipLaunchKernelGGL(k_block_krylov_init_fin, dim3(1), dim3(64), 0, st, W.gm_part.p, vg, W.sc.p, W.ctl.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_ctl, W.ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(h_sc, W.sc.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    bool stop = h_ctl[0] != 0;
    while (!stop) {
        hipLaunchKernelGGL(k_gm_cycle_init, dim3(vg), dim3(256), 0, st, n2, m, W.r.p, W.sc.p, gs, W.gm_V.p, W.ctl.p);
        for (int j = 0; j < m; ++j) {
            const double* vj = W.gm_V.p + (size_t)j * n2;
            op(vj, w, W.ctl.p);
            for (int pass = 0; pass < 2; ++pass) {
                hipLaunchKernelGGL(k_gm_dots, dim3(kGmStripes, j + 1), dim3(256), 0, st, n2, W.gm_V.p, w, W.gm_part.p, W.ctl.p);
                hipLaunchKernelGGL(k_gm_reduce, dim3(j + 1), dim3(256), 0, st, W.gm_part.p, h_pass, hcol, pass, W.ctl.p);
                hipLaunchKernelGGL(k_gm_axpy, dim3(vg), dim3(256), 0, st, n2, j + 1, W.gm_V.p, h_pass, w, gm_norm, pass, W.ctl.p);
            }
            hipLaunchKernelGGL(k_gm_hess, dim3(1), dim3(256), 0, st, j, m, gm_norm, vg, gs, W.sc.p, W.ctl.p, tol2, maxit);
            hipLaunchKernelGGL(k_gm_next, dim3(vg), dim3(256), 0, st, n2, w, gs, m, W.gm_V.p + (size_t)(j + 1) * n2, W.ctl.p);
            if (j % 10 == 9 && j + 1 < m) {
                HIPCHK(c, hipMemcpyAsync(h_ctl, W.ctl.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
                HIPCHK(c, hipStreamSynchronize(st));
                if (h_ctl[0] != 0) break;
            }
        }
        hipLaunchKernelGGL(k_gm_solve_y, dim3(1), dim3(1), 0, st, m, gs);
        hipLaunchKernelGGL(k_gm_update_x, dim3(vg), dim3(256), 0, st, n2, m, W.gm_V.p, gs, W.x.p);
        op(W.x.p, W.t.p, nullptr);
        hipLaunchKernelGGL(k_gm_residual, dim3(vg), dim3(256), 0, st, n2, W.bt.p, W.t.p, W.r.p, W.gm_part.p);
        hipLaunchKernelGGL(k_gm_cycle_fin, dim3(1), dim3(256), 0, st, W.gm_part.p, vg, W.sc.p, W.ctl.p, tol2, maxit);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(h_ctl, W.ctl.p, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipMemcpyAsync(h_sc, W.sc.p, 4 * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        stop = h_ctl[0] != 0;
    }
    return FDAPDE_OK;
}

}   // namespace fdapde_engine
#endif
