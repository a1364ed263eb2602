// las.h — launch wrappers of the LAS network's kernels (las.hip; internal, C++).  Layouts (all fp32, rows r = t*Bp + b):
//   encoder layer output  out [L*Bp][2*LAS_HE]      fw units at [0,250), bw units at [256,506), zero padding between
//   encoder gate activations act [L*Bp][2][4][LAS_HE], cell state c [L*Bp][2][LAS_HE]   (i, j, f, o after their nonlinearity)
//   pyramid input         X [L'*Bp][4*LAS_HE]        concat(out[2t'], out[2t'+1])
//   decoder step input    S [(U+1)*Bp][LAS_SW]       [attention a_{t-1} (256) | h_{t-1} (512)]
//   decoder h and context HC [U*Bp][2*LAS_HD]        [h_t (512) | context_t (512, the memory's layout)]
// The recurrent products run in the order k = 0, 1, 2, ... (one fmaf chain per output): no atomics, bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nasr {

constexpr int LAS_H = 250;        // encoder units per direction, attention layer size (networks/las.py num_hidden)
constexpr int LAS_HE = 256;       // ... padded
constexpr int LAS_G4E = 4 * LAS_H;   // encoder gate columns per direction (TF order i, j, f, o, LAS_H each)
constexpr int LAS_HD = 512;       // decoder units (2 * num_hidden = 500) padded; also the memory / attention-unit width
constexpr int LAS_G4D = 2000;     // decoder gate columns (TF order i, j, f, o, 500 each)
constexpr int LAS_SW = LAS_HE + LAS_HD;   // decoder step-input row: [a (256) | h (512)]
// memory feature q (TF order [fw 250; bw 250]) -> internal column
__host__ __device__ inline int las_memcol(int q) { return (q / LAS_H) * LAS_HE + q % LAS_H; }

// sum over a wave of 64 lanes in a fixed butterfly order (every lane gets the same result)
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// Thread k (of 512) of a decoder row's initial state: Srow [LAS_SW] = [a = 0 | h = (h_fw final; h_bw final)], crow [LAS_HD] =
// (c_fw final; c_bw final) of utterance b's top encoder layer (fw: frame L4-1, bw: frame 0); live = false: a zero row
__device__ __forceinline__ void las_final_state(const float* __restrict__ out4, const float* __restrict__ c4, int L4, int Bp, int b,
                                                bool live, int k, float* __restrict__ Srow, float* __restrict__ crow) {
  float h = 0.f, cv = 0.f;
  if (live && k < 2 * LAS_H) {
    const int d = k / LAS_H, j = k % LAS_H;
    const size_t row = (size_t)(d == 0 ? L4 - 1 : 0) * Bp + b;
    h = out4[row * (2 * LAS_HE) + d * LAS_HE + j];
    cv = c4[(row * 2 + d) * LAS_H + j];
  }
  if (k < LAS_HE) Srow[k] = 0.f;
  Srow[LAS_HE + k] = h;
  crow[k] = cv;
}

// encoder
void launch_las_enc_fwd_step(const float* xp, const float* WhF, const float* WhB, float* act, float* c, float* out, int s,
                             int L, int B, int Bp, hipStream_t st);
void launch_las_transpose_wh(const float* Wh, float* WT, hipStream_t st);
// WhTF / WhTB: [G4E][LAS_HE] transposes of the recurrent matrices
void launch_las_enc_bwd_step(const float* dout, const float* WhTF, const float* WhTB, const float* act, const float* c,
                             float* dG, float* dhc, float* dcc, int s, int L, int B, int Bp, hipStream_t st);
void launch_las_pyr_pack(const float* out, float* X, int Lh, int Bp, hipStream_t st);
void launch_las_pyr_unpack(const float* dX, float* dout, int Lh, int Bp, hipStream_t st);
// decoder
void launch_las_dec_init(const float* out4, const float* c4, const int32_t* labels, int Lmax, int L4, int B, int Bp,
                         float* S0, float* c0, int32_t* ids0, hipStream_t st);
void launch_las_dec_cell(const float* gp, const float* E, const float* bias, const int32_t* ids, const float* cprev,
                         float* act, float* c, float* Snext, float* HC, int Bp, hipStream_t st);
// attention of `rows` decoder rows, row r over the memory of utterance r / W; rows >= nrows get a zero context.  alpha
// [rows][L4] or nullptr; done: nullptr, or a word that makes the launch return at once when it is set
void launch_las_attend(const float* keys, const float* mem, const float* q, const float* v, float* alpha, float* HC, int L4,
                       int Bp, int W, int nrows, int rows, const int32_t* done, hipStream_t st);
struct LasSample { float p; uint32_t thr, key; int on; };
void launch_las_sample(const float* logits, int Cp, int C, const int32_t* labels, int Lmax, int t, int B, int Bp,
                       LasSample smp, int32_t* ids_next, int32_t* sampled, hipStream_t st);
// sequence loss: per row w*CE and d(w*CE)/dlogits; then the fixed-order sums, the loss and the 1/(sum w + 1e-12) scale
void launch_las_ce(const float* logits, const int32_t* labels, const int32_t* lablen, int Lmax, int U, int B, int Bp, int C,
                   int Cp, float* dL, float* wce, float* w, hipStream_t st);
void launch_las_loss(const float* wce, const float* w, int U, int B, int Bp, float* loss, float* nll, float* dL, int Cp,
                     hipStream_t st);
// decoder BPTT
void launch_las_add(const float* a, int lda, const float* b, int ldb, float* out, int ldo, int rows, int cols, hipStream_t st);
void launch_las_attend_bwd(const float* keys, const float* mem, const float* q, const float* v, const float* alpha,
                           const float* dHC, float* dQ, float* dkeys, float* dmem, float* dvpart, int L4, int Bp, bool first,
                           hipStream_t st);
void launch_las_dec_cell_bwd(const float* act, const float* c, const float* cprev, const float* dHC, const float* dhq,
                             const float* dSnext, float* dcc, float* dG, int Bp, bool last, hipStream_t st);
void launch_las_dec_init_bwd(const float* dS0, const float* dc0, float* dhc, float* dcc, int B, int Bp, hipStream_t st);
void launch_las_embed_grad(const float* dG, const int32_t* ids, int U, int B, int Bp, int C, float* dE, hipStream_t st);

}  // namespace nasr
