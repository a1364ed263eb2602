// ctc_harness.hip — test-only C entry points over the CTC launchers of kernels.h (ctc.hip): launch_ctc_logz,
// launch_ctc_alpha_beta in its plain and its engineered walk, launch_ctc_grad, launch_greedy and launch_mean.  Linked into
// neuralasr_amd/libnasr_kt.so with the SAME ctc.o object as libnasr.so (neuralasr_amd/build.py), so the tests run the shipped
// code objects.  The conventions of harness.hip hold: host pointers in, allocate, upload, launch on one stream in the order
// the library does (nasr_pass.hip: ctc_forward = logZ, alpha/beta; then logit_grads' launch_ctc_grad, in place over the
// logits), synchronise, download, free; -1 for refused arguments, a HIP error as its code.  Buffers the kernels write are
// pre-filled with the caller's byte (k->fill), the workspaces a pass only uses inside itself - alpha, beta, aoff, boff,
// lprobs, goff, the greedy argmax - with k->ws_fill; all of them are sized exactly as ensure_ctc_buffers (nasr_batch.hip)
// sizes them for T = Tp.  The logits of kt_ctc_pass are an in-place buffer and come in whole from the caller.
//
// What validate_batch and ensure_ctc_buffers refuse for a handle is refused here (ctc_args_ok), so that no undefined input
// reaches a kernel; label ids are held to [0, C-2] over the whole row of Lmax entries, not only the first label_len[b].
#include "../../neuralasr_amd/csrc/kernels.h"
#include "arena.h"

#include <vector>

using namespace nasr;

extern "C" {

struct KtCtc {
  int Tp, B, Bp, C, Cp, Lmax;
  float scale;    // kt_ctc_pass: the factor of the gradient (the library's 1 / B)
  int plain;      // kt_ctc_pass: 1 = lprobs and goff are withheld from CtcDims, so the plain walk runs at any C
  int ws_fill;    // byte every workspace is pre-filled with
  int fill;       // byte every output buffer is pre-filled with
};

}  // extern "C"

namespace {

// labels == NULL (greedy): the label side is not looked at
bool ctc_args_ok(const KtCtc* k, const int* seq_len, const int* labels, const int* label_len) {
  if (!k || !seq_len) return false;
  if (k->B < 1 || k->B > 64 || k->Bp != (int)rup(k->B, 16) || k->C < 2 || k->Cp != (int)rup(k->C, 32) || k->Tp < 1) return false;
  if ((double)k->Tp * k->Bp * k->Cp * 4 >= 4294967296.0) return false;       // the walks' 32-bit byte offsets
  for (int b = 0; b < k->Bp; ++b)
    if (b < k->B ? (seq_len[b] < 1 || seq_len[b] > k->Tp) : seq_len[b] != 0) return false;
  if (!labels) return true;
  if (!label_len || k->Lmax < 1 || ctc_states_per_lane(k->Lmax) > 16) return false;
  for (int b = 0; b < k->B; ++b) {
    const int L = label_len[b];
    const int* lb = labels + (size_t)b * k->Lmax;
    if (L < 0 || L > k->Lmax) return false;
    int rep = 0;
    for (int i = 0; i < k->Lmax; ++i) {
      if (lb[i] < 0 || lb[i] > k->C - 2) return false;
      if (i > 0 && i < L && lb[i] == lb[i - 1]) ++rep;
    }
    if (L + rep > seq_len[b]) return false;                                   // TF: not enough time for the target
  }
  return true;
}

CtcDims dims_of(const KtCtc* k, int Lmax) {
  CtcDims d;
  d.Tp = k->Tp; d.B = k->B; d.Bp = k->Bp; d.C = k->C; d.Cp = k->Cp; d.Lmax = Lmax;
  d.KS = ctc_states_per_lane(Lmax); d.Tws = k->Tp + 8;
  return d;
}

}  // namespace

extern "C" {

// ---- logZ, alpha / beta, the gradient.  logits [Tp*Bp][Cp]: in, and the gradient out; seq_len [Bp]; labels [B][Lmax];
// label_len [B]; logz [Tp*Bp]; nll [Bp] and logp [Bp] (the kernels write B of them).
int kt_ctc_pass(const KtCtc* k, float* logits, const int* seq_len, const int* labels, const int* label_len, float* logz,
                float* nll, double* logp) {
  if (!logits || !labels || !logz || !nll || !logp || !ctc_args_ok(k, seq_len, labels, label_len)) return -1;
  CtcDims d = dims_of(k, k->Lmax);
  const size_t B = d.B, rows = (size_t)d.Tp * d.Bp, Tws = d.Tws, KG = ctc_group_rows(d.Tws);
  // cstart / cpos as write_meta (nasr_batch.hip) builds them
  std::vector<int32_t> cstart(B * (d.C + 1), 0), cpos(B * d.Lmax, 0), scratch;
  for (size_t b = 0; b < B; ++b)
    ctc_class_positions(labels + b * d.Lmax, label_len[b], d.C, cstart.data() + b * (d.C + 1), cpos.data() + b * d.Lmax, scratch);
  Arena a;
  float* lg = a.up(logits, rows * d.Cp);
  const int* sq = a.up(seq_len, (size_t)d.Bp);
  const int* lab = a.up(labels, B * d.Lmax);
  const int* ll = a.up(label_len, B);
  const int* cs = a.up(cstart.data(), cstart.size());
  const int* cp = a.up(cpos.data(), cpos.size());
  float* lz = a.filled<float>(rows, k->fill);
  float* nl = a.filled<float>((size_t)d.Bp, k->fill);
  double* lp = a.filled<double>((size_t)d.Bp, k->fill);
  float* alpha = a.filled<float>(B * Tws * d.KS * 64, k->ws_fill);
  float* beta = a.filled<float>(B * Tws * d.KS * 64, k->ws_fill);
  double* aoff = a.filled<double>(B * Tws, k->ws_fill);
  double* boff = a.filled<double>(B * Tws, k->ws_fill);
  float* lprobs = a.filled<float>(rows * d.Cp, k->ws_fill);
  double* goff = a.filled<double>(B * 2 * KG, k->ws_fill);
  if (a.err != hipSuccess) return (int)a.err;
  if (!k->plain) { d.lprobs = lprobs; d.goff = goff; }
  launch_ctc_logz(d, lg, sq, lz, a.st);
  launch_ctc_alpha_beta(d, lg, lz, lab, ll, sq, alpha, beta, aoff, boff, nl, lp, a.st);
  launch_ctc_grad(d, lg, lz, ll, sq, cs, cp, alpha, beta, aoff, boff, lp, k->scale, a.st);
  a.down(logits, lg, rows * d.Cp); a.down(logz, lz, rows); a.down(nll, nl, (size_t)d.Bp); a.down(logp, lp, (size_t)d.Bp);
  return a.finish();
}

// ---- argmax + collapse.  ids [B][Tp], lens [Bp] (the kernel writes B of them).
int kt_ctc_greedy(const KtCtc* k, const float* logits, const int* seq_len, int* ids, int* lens) {
  if (!logits || !ids || !lens || !ctc_args_ok(k, seq_len, nullptr, nullptr)) return -1;
  const CtcDims d = dims_of(k, 1);
  const size_t rows = (size_t)d.Tp * d.Bp;
  Arena a;
  const float* lg = a.up(logits, rows * d.Cp);
  const int* sq = a.up(seq_len, (size_t)d.Bp);
  int* amax = a.filled<int>(rows, k->ws_fill);
  int* di = a.filled<int>((size_t)d.B * d.Tp, k->fill);
  int* dl = a.filled<int>((size_t)d.Bp, k->fill);
  if (a.err != hipSuccess) return (int)a.err;
  launch_greedy(d, lg, sq, amax, di, dl, a.st);
  a.down(ids, di, (size_t)d.B * d.Tp); a.down(lens, dl, (size_t)d.Bp);
  return a.finish();
}

// ---- launch_mean over v [n]; out [n_out >= 1] floats, of which the kernel writes the first
int kt_mean(const float* v, int n, float* out, int n_out, int fill) {
  if (!v || !out || n < 1 || n_out < 1) return -1;
  Arena a;
  const float* dv = a.up(v, (size_t)n);
  float* o = a.filled<float>((size_t)n_out, fill);
  if (a.err != hipSuccess) return (int)a.err;
  launch_mean(dv, n, o, a.st);
  a.down(out, o, (size_t)n_out);
  return a.finish();
}

}  // extern "C"
