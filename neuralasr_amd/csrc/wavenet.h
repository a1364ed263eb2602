// wavenet.h — launch wrappers of the WaveNet kernels (wavenet.hip): dilated 1-D convolution as im2col + fp32 GEMM
// (gemm.hip), batch norm statistics / apply / backward, the gated and residual epilogues, the moving-statistics update.
// Layout: activations are time-major rows r = t*Bp + b of `dim` channels; a tap k of rate r reads row r + (k-ks/2)*rate*Bp,
// rows outside [0, T*Bp) read zero.  Rows with b >= B (the batch padding) are written as zero everywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nasr {

struct WnRows {
  int T, B, Bp;          // real rows: t < T, b < B (frames past seq_len count: TF normalises the zero-padded batch)
  int R() const { return T * Bp; }
};

// col[r][k*D + c] = z[r + (k - KS/2)*rate*Bp][c] (zero outside [0, R))
void launch_wn_im2col(const float* z, float* col, const WnRows& rw, int D, int KS, int rate, hipStream_t st);
// dz[r][c] += sum_k dcol[r - (k - KS/2)*rate*Bp][k*D + c], k = 0..KS-1 in order
void launch_wn_col2im_add(const float* dcol, float* dz, const WnRows& rw, int D, int KS, int rate, hipStream_t st);
// Per-channel reductions over the real rows run in two levels: wn_stat_chunks(rw) chunks of rows, each summed by its own
// blocks into a workspace `ws` of WN_STAT_WS floats, then the chunks added in order (deterministic).
constexpr int WN_MAX_CHUNKS = 128;
constexpr int WN_STAT_WS = 2 * WN_MAX_CHUNKS * 256;   // channels N <= 256
int wn_stat_chunks(const WnRows& rw);
// per channel c < N <= 256 of y [R][N]: mean, then population variance (two passes), and the variance of the
// moving-statistics update (bessel: N/(N-1) * var, with N-1 taken as 1 when N = 1, as TF's fused batch norm does)
void launch_wn_bn_stats(const float* y, int N, const WnRows& rw, bool bessel, float* mean, float* var, float* vup, float* ws,
                        hipStream_t st);
// out = tanh(gamma*(y-mean)/sqrt(var+eps) + beta) [R][D]; zin != NULL: znext = out + zin; skip != NULL: skip = out
// (skip_first) or skip + out
void launch_wn_bn_tanh(const float* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                       float* out, const float* zin, float* znext, float* skip, bool skip_first, const WnRows& rw, int D,
                       hipStream_t st);
// y [R][2D]: f = tanh(BN(y[:, :D])), g = sigmoid(BN(y[:, D:])) into fg [R][2D], p = f*g into p [R][D]
void launch_wn_bn_gate(const float* y, const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                       float* fg, float* p, const WnRows& rw, int D, hipStream_t st);
// dy = (d1 + d2) * (1 - out^2)   [R][D]  (d2 may be NULL)
void launch_wn_dtanh(float* dy, const float* d1, const float* d2, const float* out, const WnRows& rw, int D, hipStream_t st);
// dy [R][2D]: dy[:, c] = dp*g*(1-f^2), dy[:, D+c] = dp*f*g*(1-g)
void launch_wn_dgate(float* dy, const float* dp, const float* fg, const WnRows& rw, int D, hipStream_t st);
// dbeta[c] = sum dy, dgamma[c] = sum dy * xhat over the real rows
void launch_wn_bn_bwd_sums(const float* y, const float* dy, const float* mean, const float* var, float eps, int N,
                           const WnRows& rw, float* dbeta, float* dgamma, float* ws, hipStream_t st);
// dy <- gamma/sqrt(var+eps) * (dy - dbeta/n - xhat*dgamma/n), n = T*B; rows b >= B <- 0
void launch_wn_bn_bwd_apply(float* dy, const float* y, const float* mean, const float* var, const float* gamma,
                            const float* dbeta, const float* dgamma, float eps, int N, const WnRows& rw, hipStream_t st);
// moving statistics of n channels: biased -= (biased - mean)*omd; mm = biased / (1 - (1-omd)^count); mv -= (mv - v)*omd
void launch_wn_bn_update(float* mm, float* mv, float* biased, const float* mean, const float* v, int n, float omd,
                         int64_t count, hipStream_t st);

}  // namespace nasr
