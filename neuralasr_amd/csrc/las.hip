// las.hip — the kernels of the LAS network (networks/las.py): the pyramidal BiLSTM encoder's recurrence and BPTT, the
// frame-pair packing between its layers, and the attention decoder's per-step cell, Bahdanau attention, scheduled
// sampling, sequence loss and their gradients.  The bulk products (input projections, keys, query, attention layer,
// projection, every weight gradient) run on gemm.hip's fp32 MFMA GEMM; nasr_las.hip orchestrates.  Layouts: las.h.
// The decoder cell and the attention kernel serve the training pass and the beam search (las_beam.hip) alike: a launch is
// over decoder rows, the training pass's utterances or the search's beams.
//
// Scheduled sampling (ScheduledEmbeddingTrainingHelper, sampling_probability p) is defined by a counter-based hash that an
// oracle can recompute (tests/test_las_host.py):
//     key  = seed + 0x9E3779B9 * (tower + 1) + 0x85EBCA6B * counter
//     u(t, b, k) = lowbias32((((t * 64 + b) * 2) + k) ^ key) >> 8                (24 bits)
// utterance b's input at step t >= 1 is sampled iff u(t, b, 0) < floor(p * 2^24); the sample is the first class k with
// u(t, b, 1) * 2^-24 < cdf_k, cdf_k = sum_{j <= k} softmax(logits_{t-1})_j summed in index order in fp32 (C - 1 when none),
// softmax_j = expf(l_j - max) / sum_i expf(l_i - max), the sum in index order.
#include "las.h"

#include <cmath>

namespace nasr {

namespace {
__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ uint32_t lowbias32(uint32_t x) {
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}
}  // namespace

// ------------------------------------------------------------------ encoder
// One launch = step s of both directions: block (b, d), thread j = unit.  The fw direction runs frame s, the bw direction
// frame L-1-s; both over every frame (sequence_length=None).  xp [L*Bp][2*G4E] = x W_x + bias of both directions.
__global__ __launch_bounds__(256) void las_enc_fwd_step_kernel(const float* __restrict__ xp, const float* __restrict__ WhF,
                                                               const float* __restrict__ WhB, float* __restrict__ act,
                                                               float* __restrict__ c, float* __restrict__ out, int s, int L,
                                                               int B, int Bp) {
  __shared__ float hs[LAS_HE];
  const int b = blockIdx.x, d = blockIdx.y, j = threadIdx.x;
  const int t = d == 0 ? s : L - 1 - s;
  const int tp = d == 0 ? t - 1 : t + 1;            // the frame whose state this step carries on from
  const bool has_prev = s > 0;
  const size_t row = (size_t)t * Bp + b;
  const size_t prow = (size_t)tp * Bp + b;
  hs[j] = has_prev && b < B ? out[prow * (2 * LAS_HE) + d * LAS_HE + j] : 0.f;
  __syncthreads();
  float* a = act + (row * 2 + d) * 4 * LAS_H;
  float* cc = c + (row * 2 + d) * LAS_H;
  float* o = out + row * (2 * LAS_HE) + d * LAS_HE;
  if (j >= LAS_H || b >= B) {
    if (j < LAS_H) {
      for (int g = 0; g < 4; ++g) a[g * LAS_H + j] = 0.f;
      cc[j] = 0.f;
    }
    o[j] = 0.f;
    return;
  }
  const float* W = d == 0 ? WhF : WhB;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
  for (int k = 0; k < LAS_H; ++k) {
    const float hk = hs[k];
    const float* w = W + (size_t)k * LAS_G4E + j;
    g0 = fmaf(hk, w[0], g0);
    g1 = fmaf(hk, w[LAS_H], g1);
    g2 = fmaf(hk, w[2 * LAS_H], g2);
    g3 = fmaf(hk, w[3 * LAS_H], g3);
  }
  const float* x = xp + row * (2 * LAS_G4E) + d * LAS_G4E + j;
  const float i_ = sigm(x[0] + g0), j_ = tanhf(x[LAS_H] + g1), f_ = sigm(x[2 * LAS_H] + g2 + 1.f), o_ = sigm(x[3 * LAS_H] + g3);
  const float cp = has_prev ? c[(prow * 2 + d) * LAS_H + j] : 0.f;
  const float cn = cp * f_ + i_ * j_;
  a[j] = i_; a[LAS_H + j] = j_; a[2 * LAS_H + j] = f_; a[3 * LAS_H + j] = o_;
  cc[j] = cn;
  o[j] = tanhf(cn) * o_;
}

void launch_las_enc_fwd_step(const float* xp, const float* WhF, const float* WhB, float* act, float* c, float* out, int s,
                             int L, int B, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_enc_fwd_step_kernel, dim3(Bp, 2), dim3(LAS_HE), 0, st, xp, WhF, WhB, act, c, out, s, L, B, Bp);
}

// WT [G4E][LAS_HE] = Wh^T of one direction (Wh [LAS_HE][G4E]): the BPTT's operand, made once per layer and pass
__global__ __launch_bounds__(256) void las_transpose_wh_kernel(const float* __restrict__ Wh, float* __restrict__ WT) {
  const int n = blockIdx.x, j = threadIdx.x;
  WT[(size_t)n * LAS_HE + j] = Wh[(size_t)j * LAS_G4E + n];
}

void launch_las_transpose_wh(const float* Wh, float* WT, hipStream_t st) {
  hipLaunchKernelGGL(las_transpose_wh_kernel, dim3(LAS_G4E), dim3(LAS_HE), 0, st, Wh, WT);
}

// BPTT step s (s = L-1 first): block (b, d), thread j.  WhTF / WhTB: the recurrent matrices transposed
// (launch_las_transpose_wh).  dhc / dcc [2][Bp][LAS_HE]: dh / dc carried into the first step
// (the final states' gradients; zero below the top layer), dcc then carries dc from launch to launch.  The recurrent part
// of dh is rebuilt from the dG row the previous launch wrote.
__global__ __launch_bounds__(256) void las_enc_bwd_step_kernel(const float* __restrict__ dout, const float* __restrict__ WhTF,
                                                               const float* __restrict__ WhTB, const float* __restrict__ act,
                                                               const float* __restrict__ c, float* __restrict__ dG,
                                                               const float* __restrict__ dhc, float* __restrict__ dcc, int s,
                                                               int L, int B, int Bp) {
  __shared__ float gs[LAS_G4E];
  const int b = blockIdx.x, d = blockIdx.y, j = threadIdx.x;
  const int t = d == 0 ? s : L - 1 - s;
  const int tn = d == 0 ? t + 1 : t - 1;            // the frame processed after this one (its dG is known)
  const int tp = d == 0 ? t - 1 : t + 1;
  const bool last = s == L - 1, first = s == 0;
  const size_t row = (size_t)t * Bp + b;
  float* g = dG + row * (2 * LAS_G4E) + d * LAS_G4E;
  if (!last)
    for (int n = j; n < LAS_G4E; n += blockDim.x) gs[n] = dG[((size_t)tn * Bp + b) * (2 * LAS_G4E) + d * LAS_G4E + n];
  __syncthreads();
  if (j >= LAS_H) return;
  float* dcp = dcc + ((size_t)d * Bp + b) * LAS_HE + j;
  if (b >= B) {
    for (int q = 0; q < 4; ++q) g[q * LAS_H + j] = 0.f;
    *dcp = 0.f;
    return;
  }
  float dh;
  if (last) {
    dh = dhc[((size_t)d * Bp + b) * LAS_HE + j];
  } else {
    const float* W = (d == 0 ? WhTF : WhTB) + j;   // the transposed matrix: lanes read consecutive units
    dh = 0.f;
    for (int n = 0; n < LAS_G4E; ++n) dh = fmaf(gs[n], W[(size_t)n * LAS_HE], dh);
  }
  dh += dout[row * (2 * LAS_HE) + d * LAS_HE + j];
  const float* a = act + (row * 2 + d) * 4 * LAS_H;
  const float i_ = a[j], j_ = a[LAS_H + j], f_ = a[2 * LAS_H + j], o_ = a[3 * LAS_H + j];
  const float cn = c[(row * 2 + d) * LAS_H + j];
  const float cp = first ? 0.f : c[(((size_t)tp * Bp + b) * 2 + d) * LAS_H + j];
  const float tc = tanhf(cn);
  const float dc = *dcp + dh * o_ * (1.f - tc * tc);
  g[j] = dc * j_ * i_ * (1.f - i_);
  g[LAS_H + j] = dc * i_ * (1.f - j_ * j_);
  g[2 * LAS_H + j] = dc * cp * f_ * (1.f - f_);
  g[3 * LAS_H + j] = dh * tc * o_ * (1.f - o_);
  *dcp = dc * f_;
}

void launch_las_enc_bwd_step(const float* dout, const float* WhTF, const float* WhTB, const float* act, const float* c,
                             float* dG, float* dhc, float* dcc, int s, int L, int B, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_enc_bwd_step_kernel, dim3(Bp, 2), dim3(LAS_HE), 0, st, dout, WhTF, WhTB, act, c, dG, dhc, dcc, s, L,
                     B, Bp);
}

// X[t'][b] = concat(out[2t'][b], out[2t'+1][b]) for t' < Lh
__global__ __launch_bounds__(256) void las_pyr_pack_kernel(const float* __restrict__ out, float* __restrict__ X, int Lh,
                                                           int Bp) {
  const int64_t n = (int64_t)Lh * Bp * 4 * LAS_HE;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % (4 * LAS_HE));
    const int64_t r = e / (4 * LAS_HE);
    const int t = (int)(r / Bp), b = (int)(r % Bp);
    const int half = k / (2 * LAS_HE);
    X[e] = out[((size_t)(2 * t + half) * Bp + b) * (2 * LAS_HE) + k % (2 * LAS_HE)];
  }
}

void launch_las_pyr_pack(const float* out, float* X, int Lh, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_pyr_pack_kernel, dim3(1024), dim3(256), 0, st, out, X, Lh, Bp);
}

// dout[t][b] = dX[t/2][b][(t%2)*512 ...] for t < 2*Lh (the next layer's odd-padding frame has no source)
__global__ __launch_bounds__(256) void las_pyr_unpack_kernel(const float* __restrict__ dX, float* __restrict__ dout, int Lh,
                                                             int Bp) {
  const int64_t n = (int64_t)2 * Lh * Bp * 2 * LAS_HE;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(e % (2 * LAS_HE));
    const int64_t r = e / (2 * LAS_HE);
    const int t = (int)(r / Bp), b = (int)(r % Bp);
    dout[e] = dX[((size_t)(t / 2) * Bp + b) * (4 * LAS_HE) + (t % 2) * 2 * LAS_HE + k];
  }
}

void launch_las_pyr_unpack(const float* dX, float* dout, int Lh, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_pyr_unpack_kernel, dim3(1024), dim3(256), 0, st, dX, dout, Lh, Bp);
}

// ------------------------------------------------------------------ decoder forward
// S0 = [a = 0 | h = (h_fw final; h_bw final)], c0 = (c_fw final; c_bw final), ids0 = labels[:, 0] (block b, 512 threads)
__global__ __launch_bounds__(512) void las_dec_init_kernel(const float* __restrict__ out4, const float* __restrict__ c4,
                                                           const int32_t* __restrict__ labels, int Lmax, int L4, int B,
                                                           int Bp, float* __restrict__ S0, float* __restrict__ c0,
                                                           int32_t* __restrict__ ids0) {
  const int b = blockIdx.x, k = threadIdx.x;
  las_final_state(out4, c4, L4, Bp, b, b < B, k, S0 + (size_t)b * LAS_SW, c0 + (size_t)b * LAS_HD);
  if (k == 0) ids0[b] = b < B ? labels[(size_t)b * Lmax] : 0;
}

void launch_las_dec_init(const float* out4, const float* c4, const int32_t* labels, int Lmax, int L4, int B, int Bp,
                         float* S0, float* c0, int32_t* ids0, hipStream_t st) {
  hipLaunchKernelGGL(las_dec_init_kernel, dim3(Bp), dim3(LAS_HD), 0, st, out4, c4, labels, Lmax, L4, B, Bp, S0, c0, ids0);
}

// the decoder LSTM cell: gp = S_t W_ah, plus the one-hot row E[id] and the bias; writes h_t into S_{t+1} and HC_t
__global__ __launch_bounds__(512) void las_dec_cell_kernel(const float* __restrict__ gp, const float* __restrict__ E,
                                                           const float* __restrict__ bias, const int32_t* __restrict__ ids,
                                                           const float* __restrict__ cprev, float* __restrict__ act,
                                                           float* __restrict__ c, float* __restrict__ Snext,
                                                           float* __restrict__ HC) {
  const int b = blockIdx.x, j = threadIdx.x;
  constexpr int HU = LAS_G4D / 4;
  float* a = act + (size_t)b * LAS_G4D;
  if (j >= HU) {
    c[(size_t)b * LAS_HD + j] = 0.f;
    Snext[(size_t)b * LAS_SW + LAS_HE + j] = 0.f;
    HC[(size_t)b * 2 * LAS_HD + j] = 0.f;
    return;
  }
  const float* g = gp + (size_t)b * LAS_G4D + j;
  const float* e = E + (size_t)ids[b] * LAS_G4D + j;
  const float* bb = bias + j;
  const float i_ = sigm(g[0] + e[0] + bb[0]), j_ = tanhf(g[HU] + e[HU] + bb[HU]);
  const float f_ = sigm(g[2 * HU] + e[2 * HU] + bb[2 * HU] + 1.f), o_ = sigm(g[3 * HU] + e[3 * HU] + bb[3 * HU]);
  const float cn = cprev[(size_t)b * LAS_HD + j] * f_ + i_ * j_;
  const float h = tanhf(cn) * o_;
  a[j] = i_; a[HU + j] = j_; a[2 * HU + j] = f_; a[3 * HU + j] = o_;
  c[(size_t)b * LAS_HD + j] = cn;
  Snext[(size_t)b * LAS_SW + LAS_HE + j] = h;
  HC[(size_t)b * 2 * LAS_HD + j] = h;
}

void launch_las_dec_cell(const float* gp, const float* E, const float* bias, const int32_t* ids, const float* cprev,
                         float* act, float* c, float* Snext, float* HC, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_dec_cell_kernel, dim3(Bp), dim3(LAS_HD), 0, st, gp, E, bias, ids, cprev, act, c, Snext, HC);
}

// Bahdanau attention of decoder row r over the memory of utterance b = r / W (block r, 4 waves): score_l = v . tanh(keys_l
// + q), alpha = softmax over all L4 frames (no memory mask), context = sum_l alpha_l mem_l into HC[r][512..].  Rows >=
// nrows get a zero context.  alpha [rows][L4] is stored unless it is nullptr; a set *done (nullptr: none) ends the launch
// at once.  Training: W = 1 and nrows = Bp (every padded row runs the body); the beam search: its W, nrows = B*W.
__global__ __launch_bounds__(256) void las_attend_kernel(const float* __restrict__ keys, const float* __restrict__ mem,
                                                         const float* __restrict__ q, const float* __restrict__ v,
                                                         float* __restrict__ alpha, float* __restrict__ HC, int L4, int Bp,
                                                         int W, int nrows, const int32_t* __restrict__ done) {
  extern __shared__ float sc[];
  if (done && *done) return;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float* ctx = HC + (size_t)r * 2 * LAS_HD + LAS_HD;
  if (r >= nrows) {
    for (int k = tid; k < LAS_HD; k += blockDim.x) ctx[k] = 0.f;
    return;
  }
  const int b = r / W;
  const float* qb = q + (size_t)r * LAS_HD;
  for (int l = w; l < L4; l += 4) {
    const float* kr = keys + ((size_t)l * Bp + b) * LAS_HD;
    float s = 0.f;
    for (int k = lane; k < LAS_HD; k += 64) s = fmaf(v[k], tanhf(kr[k] + qb[k]), s);
    s = wave_sum(s);
    if (lane == 0) sc[l] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float m = sc[0];
    for (int l = 1; l < L4; ++l) m = fmaxf(m, sc[l]);
    float z = 0.f;
    for (int l = 0; l < L4; ++l) { sc[l] = expf(sc[l] - m); z += sc[l]; }
    for (int l = 0; l < L4; ++l) sc[l] = sc[l] / z;
  }
  __syncthreads();
  if (alpha)
    for (int l = tid; l < L4; l += blockDim.x) alpha[(size_t)r * L4 + l] = sc[l];
  for (int k = tid; k < LAS_HD; k += blockDim.x) {
    float s = 0.f;
    for (int l = 0; l < L4; ++l) s = fmaf(sc[l], mem[((size_t)l * Bp + b) * LAS_HD + k], s);
    ctx[k] = s;
  }
}

void launch_las_attend(const float* keys, const float* mem, const float* q, const float* v, float* alpha, float* HC, int L4,
                       int Bp, int W, int nrows, int rows, const int32_t* done, hipStream_t st) {
  hipLaunchKernelGGL(las_attend_kernel, dim3(rows), dim3(256), (size_t)L4 * 4, st, keys, mem, q, v, alpha, HC, L4, Bp, W, nrows,
                     done);
}

// the input of step t+1: labels[:, t+1], or with probability p a sample from softmax(logits_t) (one thread per utterance)
__global__ __launch_bounds__(64) void las_sample_kernel(const float* __restrict__ logits, int Cp, int C,
                                                        const int32_t* __restrict__ labels, int Lmax, int t, int B, int Bp,
                                                        LasSample smp, int32_t* __restrict__ ids_next,
                                                        int32_t* __restrict__ sampled) {
  for (int b = threadIdx.x; b < Bp; b += blockDim.x) {
    if (b >= B) { ids_next[b] = 0; sampled[b] = 0; continue; }
    int id = labels[(size_t)b * Lmax + t + 1];
    int sm = 0;
    if (smp.on) {
      const uint32_t base = ((uint32_t)(t + 1) * 64u + (uint32_t)b) * 2u;
      const uint32_t u0 = lowbias32(base ^ smp.key) >> 8;
      if (u0 < smp.thr) {
        const uint32_t u1 = lowbias32((base + 1u) ^ smp.key) >> 8;
        const float u = (float)u1 * (1.f / 16777216.f);
        const float* l = logits + (size_t)b * Cp;
        float m = l[0];
        for (int k = 1; k < C; ++k) m = fmaxf(m, l[k]);
        float z = 0.f;
        for (int k = 0; k < C; ++k) z += expf(l[k] - m);
        float cdf = 0.f;
        id = C - 1;
        for (int k = 0; k < C; ++k) {
          cdf += expf(l[k] - m) / z;
          if (u < cdf) { id = k; break; }
        }
        sm = 1;
      }
    }
    ids_next[b] = id;
    sampled[b] = sm;
  }
}

void launch_las_sample(const float* logits, int Cp, int C, const int32_t* labels, int Lmax, int t, int B, int Bp,
                       LasSample smp, int32_t* ids_next, int32_t* sampled, hipStream_t st) {
  hipLaunchKernelGGL(las_sample_kernel, dim3(1), dim3(64), 0, st, logits, Cp, C, labels, Lmax, t, B, Bp, smp, ids_next, sampled);
}

// ------------------------------------------------------------------ sequence loss
// row r = t*Bp + b: w = (b < B && t < lablen[b]); wce = w * (logsumexp - logit[label]); dL = w * (softmax - onehot)
__global__ __launch_bounds__(64) void las_ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                    const int32_t* __restrict__ lablen, int Lmax, int B, int Bp, int C, int Cp,
                                                    float* __restrict__ dL, float* __restrict__ wce, float* __restrict__ w) {
  const int r = blockIdx.x, lane = threadIdx.x;
  const int t = r / Bp, b = r % Bp;
  const float* l = logits + (size_t)r * Cp;
  float* g = dL + (size_t)r * Cp;
  const bool on = b < B && t < lablen[b];
  if (!on) {
    for (int k = lane; k < Cp; k += 64) g[k] = 0.f;
    if (lane == 0) { wce[r] = 0.f; w[r] = 0.f; }
    return;
  }
  float m = -INFINITY;
  for (int k = lane; k < C; k += 64) m = fmaxf(m, l[k]);
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
  float z = 0.f;
  for (int k = lane; k < C; k += 64) z += expf(l[k] - m);
  z = wave_sum(z);
  const int y = labels[(size_t)b * Lmax + t];
  for (int k = lane; k < Cp; k += 64) g[k] = k < C ? expf(l[k] - m) / z - (k == y ? 1.f : 0.f) : 0.f;
  if (lane == 0) {
    wce[r] = (logf(z) + m) - l[y];
    w[r] = 1.f;
  }
}

void launch_las_ce(const float* logits, const int32_t* labels, const int32_t* lablen, int Lmax, int U, int B, int Bp, int C,
                   int Cp, float* dL, float* wce, float* w, hipStream_t st) {
  hipLaunchKernelGGL(las_ce_kernel, dim3(U * Bp), dim3(64), 0, st, logits, labels, lablen, Lmax, B, Bp, C, Cp, dL, wce, w);
}

// one block: nll[b] = sum_t wce (t ascending); loss = sum_b nll[b] / (sum w + 1e-12) (b ascending); dL *= 1 / (sum w + 1e-12)
__global__ __launch_bounds__(256) void las_loss_kernel(const float* __restrict__ wce, const float* __restrict__ w, int U,
                                                       int B, int Bp, float* __restrict__ loss, float* __restrict__ nll) {
  __shared__ float part[2][64];
  const int b = threadIdx.x;
  if (b < 64) {
    float s = 0.f, n = 0.f;
    if (b < B)
      for (int t = 0; t < U; ++t) { s += wce[(size_t)t * Bp + b]; n += w[(size_t)t * Bp + b]; }
    part[0][b] = s;
    part[1][b] = n;
    if (b < Bp) nll[b] = s;
  }
  __syncthreads();
  if (b == 0) {
    float s = 0.f, n = 0.f;
    for (int i = 0; i < B; ++i) { s += part[0][i]; n += part[1][i]; }
    const float den = n + 1e-12f;
    loss[0] = s / den;
    loss[1] = 1.f / den;
  }
}

__global__ __launch_bounds__(256) void las_scale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ s) {
  const float k = s[1];
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) x[e] *= k;
}

void launch_las_loss(const float* wce, const float* w, int U, int B, int Bp, float* loss, float* nll, float* dL, int Cp,
                     hipStream_t st) {
  hipLaunchKernelGGL(las_loss_kernel, dim3(1), dim3(256), 0, st, wce, w, U, B, Bp, loss, nll);
  hipLaunchKernelGGL(las_scale_kernel, dim3(256), dim3(256), 0, st, dL, (int64_t)U * Bp * Cp, (const float*)loss);
}

// ------------------------------------------------------------------ decoder BPTT
__global__ __launch_bounds__(256) void las_add_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b,
                                                      int ldb, float* __restrict__ out, int ldo, int rows, int cols) {
  const int64_t n = (int64_t)rows * cols;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / cols), k = (int)(e % cols);
    out[(size_t)r * ldo + k] = a[(size_t)r * lda + k] + b[(size_t)r * ldb + k];
  }
}

void launch_las_add(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int cols, hipStream_t st) {
  const int64_t n = (int64_t)rows * cols;
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(las_add_kernel, dim3(blocks), dim3(256), 0, st, a, lda, b, ldb, out, ldo, rows, cols);
}

// attention backward of utterance b at one step: dctx = dHC[b][512..]; dalpha_l = dctx . mem_l; dscore = alpha (dalpha -
// alpha . dalpha); dkeys_l += dscore_l v (1 - tau_l^2), dmem_l += alpha_l dctx (steps run in order: one writer per
// element), dq = sum_l dscore_l v (1 - tau_l^2) (l ascending), dvpart[b] = sum_l dscore_l tau_l.  first: the first
// (= last decoder) step overwrites dkeys / dmem instead of adding.
__global__ __launch_bounds__(256) void las_attend_bwd_kernel(const float* __restrict__ keys, const float* __restrict__ mem,
                                                             const float* __restrict__ q, const float* __restrict__ v,
                                                             const float* __restrict__ alpha, const float* __restrict__ dHC,
                                                             float* __restrict__ dQ, float* __restrict__ dkeys,
                                                             float* __restrict__ dmem, float* __restrict__ dvpart, int L4,
                                                             int Bp, int first) {
  extern __shared__ float sh[];
  float* da = sh;            // [L4]
  float* ds = sh + L4;       // [L4]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* dctx = dHC + (size_t)b * 2 * LAS_HD + LAS_HD;
  const float* al = alpha + (size_t)b * L4;
  for (int l = w; l < L4; l += 4) {
    const float* mr = mem + ((size_t)l * Bp + b) * LAS_HD;
    float s = 0.f;
    for (int k = lane; k < LAS_HD; k += 64) s = fmaf(dctx[k], mr[k], s);
    s = wave_sum(s);
    if (lane == 0) da[l] = s;
  }
  __syncthreads();
  if (tid == 0) {
    float dot = 0.f;
    for (int l = 0; l < L4; ++l) dot = fmaf(al[l], da[l], dot);
    for (int l = 0; l < L4; ++l) ds[l] = al[l] * (da[l] - dot);
  }
  __syncthreads();
  const float* qb = q + (size_t)b * LAS_HD;
  for (int k = tid; k < LAS_HD; k += blockDim.x) {
    const float vk = v[k], qk = qb[k], dk = dctx[k];
    float dq = 0.f, dv = 0.f;
    for (int l = 0; l < L4; ++l) {
      const size_t e = ((size_t)l * Bp + b) * LAS_HD + k;
      const float tau = tanhf(keys[e] + qk);
      const float g = ds[l] * vk * (1.f - tau * tau);
      dq += g;
      dv = fmaf(ds[l], tau, dv);
      const float dm = al[l] * dk;
      dkeys[e] = first ? g : dkeys[e] + g;
      dmem[e] = first ? dm : dmem[e] + dm;
    }
    dQ[(size_t)b * LAS_HD + k] = dq;
    dvpart[(size_t)b * LAS_HD + k] = dv;
  }
}

void launch_las_attend_bwd(const float* keys, const float* mem, const float* q, const float* v, const float* alpha,
                           const float* dHC, float* dQ, float* dkeys, float* dmem, float* dvpart, int L4, int Bp, bool first,
                           hipStream_t st) {
  hipLaunchKernelGGL(las_attend_bwd_kernel, dim3(Bp), dim3(256), (size_t)2 * L4 * 4, st, keys, mem, q, v, alpha, dHC, dQ,
                     dkeys, dmem, dvpart, L4, Bp, first ? 1 : 0);
}

// decoder cell backward at step t: dh = dHC_h + dq W_q^T + dS_{t+1}[h]; dcc carries dc (last: this is the last step, the
// carry starts at zero); dG [Bp][G4D]
__global__ __launch_bounds__(512) void las_dec_cell_bwd_kernel(const float* __restrict__ act, const float* __restrict__ c,
                                                               const float* __restrict__ cprev, const float* __restrict__ dHC,
                                                               const float* __restrict__ dhq, const float* __restrict__ dSnext,
                                                               float* __restrict__ dcc, float* __restrict__ dG, int last) {
  const int b = blockIdx.x, j = threadIdx.x;
  constexpr int HU = LAS_G4D / 4;
  float* dcp = dcc + (size_t)b * LAS_HD + j;
  if (j >= HU) { *dcp = 0.f; return; }
  const float dh = dHC[(size_t)b * 2 * LAS_HD + j] + dhq[(size_t)b * LAS_HD + j] +
                   (last ? 0.f : dSnext[(size_t)b * LAS_SW + LAS_HE + j]);
  const float* a = act + (size_t)b * LAS_G4D;
  const float i_ = a[j], j_ = a[HU + j], f_ = a[2 * HU + j], o_ = a[3 * HU + j];
  const float cn = c[(size_t)b * LAS_HD + j], cp = cprev[(size_t)b * LAS_HD + j];
  const float tc = tanhf(cn);
  const float dc = (last ? 0.f : *dcp) + dh * o_ * (1.f - tc * tc);
  float* g = dG + (size_t)b * LAS_G4D;
  g[j] = dc * j_ * i_ * (1.f - i_);
  g[HU + j] = dc * i_ * (1.f - j_ * j_);
  g[2 * HU + j] = dc * cp * f_ * (1.f - f_);
  g[3 * HU + j] = dh * tc * o_ * (1.f - o_);
  *dcp = dc * f_;
}

void launch_las_dec_cell_bwd(const float* act, const float* c, const float* cprev, const float* dHC, const float* dhq,
                             const float* dSnext, float* dcc, float* dG, int Bp, bool last, hipStream_t st) {
  hipLaunchKernelGGL(las_dec_cell_bwd_kernel, dim3(Bp), dim3(LAS_HD), 0, st, act, c, cprev, dHC, dhq, dSnext, dcc, dG,
                     last ? 1 : 0);
}

// the initial decoder state's gradient back to the top encoder layer's final states: dhc / dcc [2][Bp][LAS_HE]
__global__ __launch_bounds__(256) void las_dec_init_bwd_kernel(const float* __restrict__ dS0, const float* __restrict__ dc0,
                                                               float* __restrict__ dhc, float* __restrict__ dcc, int B) {
  const int b = blockIdx.x, d = blockIdx.y, j = threadIdx.x;
  const size_t o = ((size_t)d * gridDim.x + b) * LAS_HE + j;
  if (j >= LAS_H || b >= B) { dhc[o] = 0.f; dcc[o] = 0.f; return; }
  dhc[o] = dS0[(size_t)b * LAS_SW + LAS_HE + d * LAS_H + j];
  dcc[o] = dc0[(size_t)b * LAS_HD + d * LAS_H + j];
}

void launch_las_dec_init_bwd(const float* dS0, const float* dc0, float* dhc, float* dcc, int B, int Bp, hipStream_t st) {
  hipLaunchKernelGGL(las_dec_init_bwd_kernel, dim3(Bp, 2), dim3(LAS_HE), 0, st, dS0, dc0, dhc, dcc, B);
}

// dE[c][n] = sum over (t ascending, b ascending, b < B) with ids[t][b] == c of dG[t][b][n]
__global__ __launch_bounds__(256) void las_embed_grad_kernel(const float* __restrict__ dG, const int32_t* __restrict__ ids,
                                                             int U, int B, int Bp, int C, float* __restrict__ dE) {
  const int c = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= LAS_G4D) return;
  float s = 0.f;
  for (int t = 0; t < U; ++t)
    for (int b = 0; b < B; ++b)
      if (ids[(size_t)t * Bp + b] == c) s += dG[((size_t)t * Bp + b) * LAS_G4D + n];
  dE[(size_t)c * LAS_G4D + n] = s;
}

void launch_las_embed_grad(const float* dG, const int32_t* ids, int U, int B, int Bp, int C, float* dE, hipStream_t st) {
  hipLaunchKernelGGL(las_embed_grad_kernel, dim3((LAS_G4D + 255) / 256, C), dim3(256), 0, st, dG, ids, U, B, Bp, C, dE);
}

}  // namespace nasr
