// rec_harness.hip — test-only C entry points over the recurrence launchers of kernels.h (lstm.hip, lstm_persist.hip,
// lstm_wide.hip).  Linked into neuralasr_amd/libnasr_kt.so with the SAME lstm.o / lstm_persist.o / lstm_wide.o objects as
// libnasr.so (neuralasr_amd/build.py), so the tests run the shipped code objects; no test hook is set (NASR_TEST_HOOKS
// stays unset) and nothing is injected.  The conventions of harness.hip hold: host pointers in, allocate, upload, launch
// on one stream in the order the library does (nasr_pass.hip: step_window, nasr_rec.hip: rec_scale_jobs / rec_images /
// rec_launch), synchronise, download, free; -1 for refused arguments, a HIP error as its code.  Buffers the kernels
// write are pre-filled with the caller's byte; `gates` of a forward call is an in-place buffer and comes in whole from the
// caller.  The resident kernels' XcdCtl::error, the sticky word and the fault float come back in status[3]; a non-zero
// word is the test's failure - nothing is retried.
//
// Layout of every argument (kernels.h): canonical U [D][Hp][4Hp] (column 4j+g), rows r = t*Bp + b, gates / dG [R][D*4Hp],
// c / out / dOut [R][D*Hp], seq_len [Bp] with 0 in the rows b >= B.
#include "../../neuralasr_amd/csrc/kernels.h"
#include "arena.h"

#include <vector>

using namespace nasr;

namespace {

bool dims_ok(const LstmDims& dm, const int* seq_len) {
  if (dm.T < 1 || dm.B < 1 || dm.Bp != (int)rup(dm.B, 16) || dm.Bp > 64 || dm.Hp < 64 || dm.Hp % 64 || dm.H < 1 || dm.H > dm.Hp ||
      (dm.D != 1 && dm.D != 2) || !seq_len)
    return false;
  if ((double)dm.T * dm.Bp * dm.D * 4 * dm.Hp >= 4294967296.0) return false;      // 32-bit element offsets of the resident kernels
  for (int b = 0; b < dm.Bp; ++b)
    if (seq_len[b] < 0 || seq_len[b] > dm.T || (b >= dm.B && seq_len[b] != 0)) return false;
  return true;
}

struct Status {       // what a resident kernel reports: ctl->error, the host-mapped sticky word, the fault float
  unsigned* sticky = nullptr;
  float* fault = nullptr;
  Status(Arena& a) {
    a.chk(hipHostMalloc(reinterpret_cast<void**>(&sticky), 64, hipHostMallocMapped));
    if (sticky) *sticky = 0;
    fault = a.filled<float>(1, 0);
  }
  ~Status() { if (sticky) (void)hipHostFree(sticky); }
  // after the stream is synchronised
  void report(Arena& a, const XcdCtl* ctl, unsigned* status) {
    unsigned err = 0xFFFFFFFFu;
    float f = -1.f;
    a.chk(hipMemcpy(&err, &ctl->error, 4, hipMemcpyDeviceToHost));
    a.chk(hipMemcpy(&f, fault, 4, hipMemcpyDeviceToHost));
    status[0] = err;
    status[1] = sticky ? *reinterpret_cast<volatile unsigned*>(sticky) : 0xFFFFFFFFu;
    status[2] = f == 0.f ? 0u : 1u;
  }
};

}  // namespace

extern "C" {

struct KtRec {
  int T, B, Bp, H, Hp, D;
  float forget_bias;
  int f16;        // persistent forward: 1 = two fp16 planes of U under column scales, 0 = fp32 (cinv == NULL)
  int lean;       // persistent BPTT: the launch that declares 24 KB of LDS
  int parts;      // persistent BPTT: 1 = rowpart / colpart are taken
  int fill;
};

// floats of rowpart + colpart as the library sizes its dgmax buffer
unsigned long long kt_persist_dgmax_floats(int T, int Bp, int Hp, int D) { return persist_dgmax_floats(T, Bp, Hp, D); }

// ---- lstm.hip, forward: launch_repack_u, then the window of T steps by lstm_steps_fwd, the runner every pass of the
// library goes through (nasr_pass.hip).  state (or NULL): [D][B][2][H] (c, then h) - the window then continues from the
// images launch_stream_load_state builds, one direction at a time.  gates: pre-activations in, activations out, in place.
int kt_lstm_step_fwd(const KtRec* k, const float* U, float* gates, float* cbuf, float* out, const int* seq_len, const float* state) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !out || !dims_ok(dm, seq_len)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4, hs = (size_t)dm.D * dm.Bp * dm.Hp;
  Arena a;
  const float* dU = a.up(U, dm.D * nU);
  float* Uf = a.filled<float>(dm.D * nU, 0xFF);
  float* Ub = a.filled<float>(dm.D * nU, 0xFF);
  StepWindow w{};
  w.dm = dm; w.Uf = Uf; w.Ub = Ub; w.forget_bias = k->forget_bias;
  w.gates = a.up(gates, R * dm.D * N4);
  w.cbuf = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  w.out = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  w.seq_len = a.up(seq_len, dm.Bp);
  w.hstate = a.filled<float>(2 * hs, 0xFF);                       // NaN until written
  float* cimg = state ? a.filled<float>(hs, 0xFF) : nullptr;
  w.c0 = cimg;
  const float* st8 = a.up(state, (size_t)dm.D * dm.B * 2 * dm.H);
  if (a.err != hipSuccess) return (int)a.err;
  for (int d = 0; d < dm.D; ++d) launch_repack_u(dU + d * nU, Uf + d * nU, Ub + d * nU, dm.Hp, a.st);
  if (state)
    for (int d = 0; d < dm.D; ++d)
      launch_stream_load_state(st8 + (size_t)d * dm.B * 2 * dm.H, w.hstate + (size_t)d * dm.Bp * dm.Hp, cimg + (size_t)d * dm.Bp * dm.Hp,
                               dm.B, dm.H, dm.Bp, dm.Hp, a.st);
  lstm_steps_fwd(w, 0, dm.T, a.st);
  a.down(gates, w.gates, R * dm.D * N4); a.down(cbuf, w.cbuf, R * dm.D * dm.Hp); a.down(out, w.out, R * dm.D * dm.Hp);
  return a.finish();
}

// ---- lstm.hip, BPTT: the window's steps T-1 .. 0 by lstm_steps_bwd (it zeroes the first partial-sum and dc images); Hp <=
// 512 in one launch per step, the two-launch form above it.  gates = the saved activations.  c0 (or NULL): [D][Bp][Hp],
// the carried c the forward window started from - step 0 then runs in its carry form.
static int step_bwd(const KtRec* k, const float* U, const float* gates, const float* cbuf, const float* dout, float* dgbuf,
                    const int* seq_len, const float* c0) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !dout || !dgbuf || !dims_ok(dm, seq_len)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4, hs = (size_t)dm.D * dm.Bp * dm.Hp;
  const size_t ps = (size_t)dm.D * lstm_bwd_partials(dm.Hp) * dm.Bp * dm.Hp;
  Arena a;
  const float* dU = a.up(U, dm.D * nU);
  float* Uf = a.filled<float>(dm.D * nU, 0xFF);
  float* Ub = a.filled<float>(dm.D * nU, 0xFF);
  StepWindow w{};
  w.dm = dm; w.Uf = Uf; w.Ub = Ub; w.forget_bias = k->forget_bias;
  w.gates = a.up(gates, R * dm.D * N4);                           // (BPTT only reads them)
  w.cbuf = a.up(cbuf, R * dm.D * dm.Hp);
  w.dout = a.up(dout, R * dm.D * dm.Hp);
  w.dg = a.filled<float>(R * dm.D * N4, k->fill);
  w.seq_len = a.up(seq_len, dm.Bp);
  w.partial = a.filled<float>(2 * ps, 0xFF);
  w.dcstate = a.filled<float>(2 * hs, 0xFF);
  w.c0 = a.up(c0, hs);
  if (a.err != hipSuccess) return (int)a.err;
  for (int d = 0; d < dm.D; ++d) launch_repack_u(dU + d * nU, Uf + d * nU, Ub + d * nU, dm.Hp, a.st);
  lstm_steps_bwd(w, 0, dm.T, a.st);
  a.down(dgbuf, w.dg, R * dm.D * N4);
  return a.finish();
}
// (two entry points, so that kt_lstm_step_bwd keeps the arguments every caller of it has ever passed)
int kt_lstm_step_bwd(const KtRec* k, const float* U, const float* gates, const float* cbuf, const float* dout, float* dgbuf,
                     const int* seq_len) {
  return step_bwd(k, U, gates, cbuf, dout, dgbuf, seq_len, nullptr);
}
int kt_lstm_step_bwd_carry(const KtRec* k, const float* U, const float* gates, const float* cbuf, const float* dout, float* dgbuf,
                           const int* seq_len, const float* c0) {
  return c0 ? step_bwd(k, U, gates, cbuf, dout, dgbuf, seq_len, c0) : -1;
}

// the operand images of the persistent kind as repack() builds them: column scales by launch_tph_scales_batch (the jobs
// of rec_scale_jobs) when the forward image holds fp16 planes, then launch_repack_persist
static bool persist_images(Arena& a, const LstmDims& dm, const float* dU, bool f16, float** Upf, float** Upb, float** cinv) {
  const size_t N4 = (size_t)4 * dm.Hp, nU = (size_t)dm.Hp * N4;
  if (!a.chk(persist_prepare())) return false;
  *Upf = a.filled<float>(dm.D * persist_image_floats(dm.Hp, false), 0xFF);
  *Upb = a.filled<float>(dm.D * persist_image_floats(dm.Hp, true), 0xFF);
  float* cs = nullptr;
  *cinv = nullptr;
  if (f16) {
    cs = a.filled<float>(dm.D * N4, 0xFF);
    *cinv = a.filled<float>(dm.D * N4, 0xFF);
    std::vector<TphScaleJob> jobs;
    for (int d = 0; d < dm.D; ++d)
      jobs.push_back({dU + d * nU, dm.Hp, (int)N4, (int)N4, nullptr, nullptr, cs + d * N4, *cinv + d * N4});
    float* ws = a.filled<float>(tph_scale_batch_ws_floats(jobs.data(), (int)jobs.size()), 0xFF);
    if (a.err != hipSuccess) return false;
    launch_tph_scales_batch(jobs.data(), (int)jobs.size(), ws, a.st);
  }
  if (a.err != hipSuccess) return false;
  const int64_t offs[2] = {0, (int64_t)nU};
  launch_repack_persist(dU, offs, dm.D, *Upf, *Upb, dm.Hp, cs, a.st);
  return true;
}

// ---- lstm_persist.hip, forward: persist_prepare, the images, ctl and the head of the exchange buffer cleared as the
// forward pass clears them, one launch with ctl_zeroed.  status[3]: error word, sticky word, fault != 0.
int kt_lstm_persist_fwd(const KtRec* k, const float* U, float* gates, float* cbuf, float* out, const int* seq_len, unsigned* status) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !out || !status || !dims_ok(dm, seq_len) || !persist_supported(dm.Hp)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4;
  Arena a;
  Status stt(a);
  const float* dU = a.up(U, dm.D * nU);
  float *Upf, *Upb, *cinv;
  if (!persist_images(a, dm, dU, k->f16 != 0, &Upf, &Upb, &cinv)) return (int)a.err;
  float* g = a.up(gates, R * dm.D * N4);
  float* c = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  float* o = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  const int* sq = a.up(seq_len, dm.Bp);
  float* xch = a.filled<float>(persist_xch_floats(dm.Hp), 0xFF);
  PersistCtl* ctl = a.filled<PersistCtl>(1, 0xFF);
  if (a.err != hipSuccess) return (int)a.err;
  a.chk(hipMemsetAsync(ctl, 0, sizeof(PersistCtl), a.st));
  a.chk(hipMemsetAsync(xch, 0, persist_hx_bytes(dm.Hp), a.st));
  launch_lstm_persist_fwd(dm, Upf, cinv, g, c, o, sq, xch, ctl, stt.sticky, stt.fault, k->forget_bias, a.st, true);
  a.down(gates, g, R * dm.D * N4); a.down(cbuf, c, R * dm.D * dm.Hp); a.down(out, o, R * dm.D * dm.Hp);
  const int rc = a.finish();
  if (rc == 0) stt.report(a, ctl, status);
  return (int)a.err;
}

// ---- lstm_persist.hip, BPTT: the same set-up, ctl and the partial-sum buffers cleared as the backward pass clears them.
// rowpart [D*32][T*Bp] / colpart [8/D][D*4Hp] (k->parts; else both NULL and the launch takes no maxima).
int kt_lstm_persist_bwd(const KtRec* k, const float* U, const float* gates, const float* cbuf, const float* dout, float* dgbuf,
                        float* rowpart, float* colpart, const int* seq_len, unsigned* status) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !dout || !dgbuf || !status || !dims_ok(dm, seq_len) || !persist_supported(dm.Hp)) return -1;
  if (k->parts && (!rowpart || !colpart)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4;
  const size_t nrp = (size_t)dm.D * 32 * R, ncp = (size_t)(8 / dm.D) * dm.D * N4;
  Arena a;
  Status stt(a);
  const float* dU = a.up(U, dm.D * nU);
  float *Upf, *Upb, *cinv;
  if (!persist_images(a, dm, dU, false, &Upf, &Upb, &cinv)) return (int)a.err;
  const float* g = a.up(gates, R * dm.D * N4);
  const float* c = a.up(cbuf, R * dm.D * dm.Hp);
  const float* dO = a.up(dout, R * dm.D * dm.Hp);
  float* dg = a.filled<float>(R * dm.D * N4, k->fill);
  float* rp = k->parts ? a.filled<float>(nrp, k->fill) : nullptr;
  float* cp = k->parts ? a.filled<float>(ncp, k->fill) : nullptr;
  const int* sq = a.up(seq_len, dm.Bp);
  float* xch = a.filled<float>(persist_xch_floats(dm.Hp), 0xFF);
  PersistCtl* ctl = a.filled<PersistCtl>(1, 0xFF);
  if (a.err != hipSuccess) return (int)a.err;
  a.chk(hipMemsetAsync(ctl, 0, sizeof(PersistCtl), a.st));
  a.chk(hipMemsetAsync(xch, 0, persist_px_bytes(), a.st));
  launch_lstm_persist_bwd(dm, Upb, g, dg, c, dO, sq, xch, ctl, stt.sticky, stt.fault, a.st, true, rp, cp, k->lean != 0);
  a.down(dgbuf, dg, R * dm.D * N4);
  if (k->parts) { a.down(rowpart, rp, nrp); a.down(colpart, cp, ncp); }
  const int rc = a.finish();
  if (rc == 0) stt.report(a, ctl, status);
  return (int)a.err;
}

// ---- lstm_wide.hip, forward (Hp = 2048): wide_prepare, both scale sets by launch_tph_scales_batch (the jobs of
// rec_scale_jobs: row scales too), launch_repack_wide, then one launch per direction as rec_launch does; the launcher
// clears ctl, the inboxes and the h buffers itself.  status: the error word of the LAST direction's launch (each launch
// clears ctl), the sticky word - which keeps the first cause of either - and the fault float.
int kt_lstm_wide_fwd(const KtRec* k, const float* U, float* gates, float* cbuf, float* out, const int* seq_len, unsigned* status) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !out || !status || !dims_ok(dm, seq_len) || !wide_supported(dm.Hp, dm.Bp)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4;
  Arena a;
  Status stt(a);
  if (!a.chk(wide_prepare())) return (int)a.err;
  const float* dU = a.up(U, dm.D * nU);
  float* cs = a.filled<float>(dm.D * N4, 0xFF);
  float* cinv = a.filled<float>(dm.D * N4, 0xFF);
  float* rs = a.filled<float>((size_t)dm.D * dm.Hp, 0xFF);
  float* rinv = a.filled<float>((size_t)dm.D * dm.Hp, 0xFF);
  unsigned char* Uw = a.filled<unsigned char>(dm.D * wide_image_bytes(dm.Hp), 0xFF);
  std::vector<TphScaleJob> jobs;
  for (int d = 0; d < dm.D; ++d)
    jobs.push_back({dU + d * nU, dm.Hp, (int)N4, (int)N4, rs + (size_t)d * dm.Hp, rinv + (size_t)d * dm.Hp, cs + d * N4, cinv + d * N4});
  float* ws = a.filled<float>(tph_scale_batch_ws_floats(jobs.data(), (int)jobs.size()), 0xFF);
  float* g = a.up(gates, R * dm.D * N4);
  float* c = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  float* o = a.filled<float>(R * dm.D * dm.Hp, k->fill);
  const int* sq = a.up(seq_len, dm.Bp);
  void* hx = a.filled<unsigned char>(wide_hx_bytes(64), 0xFF);
  float* part = a.filled<float>(wide_part_bytes(64) / 4, 0x00);
  WideCtl* ctl = a.filled<WideCtl>(1, 0xFF);
  if (a.err != hipSuccess) return (int)a.err;
  launch_tph_scales_batch(jobs.data(), (int)jobs.size(), ws, a.st);
  for (int d = 0; d < dm.D; ++d) launch_repack_wide(dU + d * nU, cs + d * N4, Uw + d * wide_image_bytes(dm.Hp), dm.Hp, a.st);
  for (int d = 0; d < dm.D; ++d)
    launch_lstm_wide_fwd(dm, d, Uw + d * wide_image_bytes(dm.Hp), cinv + d * N4, g, c, o, sq, hx, part, ctl, stt.sticky, stt.fault,
                         k->forget_bias, a.st);
  a.down(gates, g, R * dm.D * N4); a.down(cbuf, c, R * dm.D * dm.Hp); a.down(out, o, R * dm.D * dm.Hp);
  const int rc = a.finish();
  if (rc == 0) stt.report(a, ctl, status);
  return (int)a.err;
}

// ---- lstm_wide.hip, BPTT (Hp = 2048): wide_prepare, both scale sets, launch_repack_wide_bwd, launch_wide_row_scales over
// dOut, then one launch per direction as rec_launch does (the launcher sets ctl, the inboxes and the partial-sum buffer).
// status as kt_lstm_wide_fwd; bit 2 of either word = dG beyond its fp16 planes.
int kt_lstm_wide_bwd(const KtRec* k, const float* U, const float* gates, const float* cbuf, const float* dout, float* dgbuf,
                     const int* seq_len, unsigned* status) {
  const LstmDims dm{k->T, k->B, k->Bp, k->H, k->Hp, k->D};
  if (!U || !gates || !cbuf || !dout || !dgbuf || !status || !dims_ok(dm, seq_len) || !wide_supported(dm.Hp, dm.Bp)) return -1;
  const size_t N4 = (size_t)4 * dm.Hp, R = (size_t)dm.T * dm.Bp, nU = (size_t)dm.Hp * N4;
  Arena a;
  Status stt(a);
  if (!a.chk(wide_prepare())) return (int)a.err;
  const float* dU = a.up(U, dm.D * nU);
  float* cs = a.filled<float>(dm.D * N4, 0xFF);
  float* cinv = a.filled<float>(dm.D * N4, 0xFF);
  float* rs = a.filled<float>((size_t)dm.D * dm.Hp, 0xFF);
  float* rinv = a.filled<float>((size_t)dm.D * dm.Hp, 0xFF);
  unsigned char* Uwb = a.filled<unsigned char>(dm.D * wide_image_bytes(dm.Hp), 0xFF);
  std::vector<TphScaleJob> jobs;
  for (int d = 0; d < dm.D; ++d)
    jobs.push_back({dU + d * nU, dm.Hp, (int)N4, (int)N4, rs + (size_t)d * dm.Hp, rinv + (size_t)d * dm.Hp, cs + d * N4, cinv + d * N4});
  float* ws = a.filled<float>(tph_scale_batch_ws_floats(jobs.data(), (int)jobs.size()), 0xFF);
  const float* g = a.up(gates, R * dm.D * N4);
  const float* c = a.up(cbuf, R * dm.D * dm.Hp);
  const float* dO = a.up(dout, R * dm.D * dm.Hp);
  float* dg = a.filled<float>(R * dm.D * N4, k->fill);
  const int* sq = a.up(seq_len, dm.Bp);
  float* srow = a.filled<float>(2 * 64, 0xFF);
  float* inbox = a.filled<float>(wide_part_bytes(64) / 4, 0x00);
  void* px = a.filled<unsigned char>(wide_px_bytes(64), 0x00);
  WideCtl* ctl = a.filled<WideCtl>(1, 0xFF);
  if (a.err != hipSuccess) return (int)a.err;
  launch_tph_scales_batch(jobs.data(), (int)jobs.size(), ws, a.st);
  for (int d = 0; d < dm.D; ++d) launch_repack_wide_bwd(dU + d * nU, rs + (size_t)d * dm.Hp, Uwb + d * wide_image_bytes(dm.Hp), dm.Hp, a.st);
  launch_wide_row_scales(dm, dO, sq, srow, a.st);
  for (int d = 0; d < dm.D; ++d)
    launch_lstm_wide_bwd(dm, d, Uwb + d * wide_image_bytes(dm.Hp), rinv + (size_t)d * dm.Hp, srow, g, dg, c, dO, sq, inbox, px, ctl,
                         stt.sticky, stt.fault, a.st);
  a.down(dgbuf, dg, R * dm.D * N4);
  const int rc = a.finish();
  if (rc == 0) stt.report(a, ctl, status);
  return (int)a.err;
}

}  // extern "C"
