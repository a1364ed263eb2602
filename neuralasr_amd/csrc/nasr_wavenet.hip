// nasr_wavenet.hip — the WaveNet CTC network of the reference (networks/wavenet.py): a 1x1 convolution with batch norm and
// tanh in front, num_blocks x |rates| residual blocks (gated dilated convolutions of kernel size 7, each with batch norm, a
// 1x1 convolution with batch norm and tanh, residual and skip outputs), a 1x1 convolution with batch norm and tanh over the
// skip sum and a last 1x1 convolution to the classes.  Every convolution is bias-free.  This file holds the handle's
// create call, parameter layout, buffers, batch-norm state and the forward / backward pass; the kernels are in wavenet.hip
// and gemm.hip.  Everything else (opening and finishing the handle, batches, CTC, decoders, Adam, gradient exchange) is the common code.
#include "nasr_ctx.h"
#include "wavenet.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

struct WnState {
  nasr_wavenet_cfg cfg;
  int D = 128, KS = 7, nblk = 0, S = 0;
  std::vector<int> rate;                      // per block: its dilation rate
  float eps = 1e-3f, omd = 0.01f;             // BN epsilon, 1 - decay
  // internal parameter layout (floats from P): conv_in W [Fp][D]; per block W_filter|W_gate interleaved [KS*D][2D], conv_out
  // W [D][D]; conv_1 W [D][D]; conv_2 W [D][Cp].  BN site s has beta at off_beta[s], gamma at off_gamma[s]; a block's
  // filter and gate sites are adjacent (beta [2D], gamma [2D]), so the gated epilogue reads one 2D-channel vector each.
  int64_t off_win = 0, off_w1 = 0, off_w2 = 0;
  std::vector<int64_t> off_wfg, off_wo, off_beta, off_gamma;
  std::vector<char> bessel;                   // per site: the update uses N/(N-1) var (1x1 convs: fused batch norm)
  // BN state [S][D] and the update count (zero_debias_moving_mean's local_step)
  DevPtr<float> mm, mv, biased;
  int64_t count = 0;
  bool hold = false;                          // training passes leave the update to nasr_wavenet_apply_bn_stats
  // the batch statistics of the last training pass [S][D]: mean, population variance, variance of the update
  DevPtr<float> bmean, bvar, bvup;
  bool have_stats = false;
  DevPtr<float> ws;                           // chunk partials of the per-channel reductions (WN_STAT_WS floats)
  // activations of the resident batch, rows R = T*Bp
  DevBuf Y0, Z, YFG, FG, Pm, Yo, O, skip, Y1, S2, col, dcol, dz, dskip, dy, dp;
  int site_filter(int j) const { return 1 + 3 * j; }
  int site_out(int j) const { return 3 + 3 * j; }
};

// Parameter names, TF order, and the map into the internal layout (nasr_tensor_info, nasr_get/set_params).
int wn_layout(nasr_ctx* h) {
  WnState& w = *h->wn;
  const int D = w.D, KS = w.KS;
  h->F = w.cfg.feature_size;
  h->C = w.cfg.num_classes;
  h->Fp = rup(h->F, 32);
  h->Cp = rup(h->C, 32);
  w.S = 2 + 3 * w.nblk;
  w.off_wfg.assign(w.nblk, 0); w.off_wo.assign(w.nblk, 0);
  w.off_beta.assign(w.S, 0); w.off_gamma.assign(w.S, 0); w.bessel.assign(w.S, 1);
  int64_t off = 0;
  auto bn = [&](int s, int n) {   // n sites' betas, then their gammas
    for (int i = 0; i < n; ++i) w.off_beta[s + i] = off + (int64_t)i * D;
    off += (int64_t)n * D;
    for (int i = 0; i < n; ++i) w.off_gamma[s + i] = off + (int64_t)i * D;
    off += (int64_t)n * D;
  };
  w.off_win = off; off += (int64_t)h->Fp * D;
  bn(0, 1);
  for (int j = 0; j < w.nblk; ++j) {
    w.off_wfg[j] = off; off += (int64_t)KS * D * 2 * D;
    bn(w.site_filter(j), 2);
    w.bessel[w.site_filter(j)] = w.bessel[w.site_filter(j) + 1] = 0;   // 5-D input: the non-fused batch norm
    w.off_wo[j] = off; off += (int64_t)D * D;
    bn(w.site_out(j), 1);
  }
  w.off_w1 = off; off += (int64_t)D * D;
  bn(w.S - 1, 1);
  w.off_w2 = off; off += (int64_t)D * h->Cp;
  h->np_int = off;

  h->tensors.clear();
  h->tf2int.clear();
  int64_t tf = 0;
  auto add = [&](const std::string& name, int64_t rows, int64_t cols, int64_t base, int64_t ld) {
    h->tensors.push_back({name, tf, rows, cols});
    for (int64_t r = 0; r < rows; ++r)
      for (int64_t c = 0; c < cols; ++c) h->tf2int.push_back((int32_t)(base + r * ld + c));
    tf += rows * cols;
  };
  auto add_bn = [&](const std::string& scope, int s) {
    add(scope + "/BatchNorm/beta", D, 1, w.off_beta[s], 1);
    add(scope + "/BatchNorm/gamma", D, 1, w.off_gamma[s], 1);
  };
  add("front/conv_in/W", h->F, D, w.off_win, D);
  add_bn("front/conv_in", 0);
  for (int j = 0; j < w.nblk; ++j) {
    const int blk = j / w.cfg.num_rates;
    const std::string name = "block_" + std::to_string(blk) + "_" + std::to_string(w.rate[j]);
    const std::string f = name + "/conv_filter" + name, g = name + "/conv_gate" + name, o = name + "/conv_out" + name;
    add(f + "/W", (int64_t)KS * D, D, w.off_wfg[j], 2 * D);
    add_bn(f, w.site_filter(j));
    add(g + "/W", (int64_t)KS * D, D, w.off_wfg[j] + D, 2 * D);
    add_bn(g, w.site_filter(j) + 1);
    add(o + "/W", D, D, w.off_wo[j], D);
    add_bn(o, w.site_out(j));
  }
  add("logit/conv_1/W", D, D, w.off_w1, D);
  add_bn("logit/conv_1", w.S - 1);
  add("logit/conv_2/W", D, h->C, w.off_w2, h->Cp);
  h->np_tf = tf;
  return NASR_OK;
}

int wn_ensure_shape(nasr_ctx* h, int B, int T, int Lmax) {
  WnState& w = *h->wn;
  const int Bp = rup(B, 16);
  const size_t R = (size_t)T * Bp;
  const int D = w.D;
  bool grew = false, ok = true;
  // the common parts: the CTC lattice's buffers (as for the LSTM handles) and the features
  const int KSa = ensure_ctc_buffers(h, B, Bp, T, T, Lmax, &grew);
  if (KSa < 0) return KSa;
  ok &= h->X0.ensure(R * h->Fp * 4, &grew);
  ok &= h->seqbuf.ensure((size_t)Bp * 4, &grew);
  // the WaveNet's activations (kept for the backward pass) and scratch
  const size_t a = R * D * 4, nb = (size_t)std::max(w.nblk, 1);
  ok &= w.Y0.ensure(a, &grew) && w.Z.ensure((nb + 1) * a, &grew);
  ok &= w.YFG.ensure(nb * 2 * a, &grew) && w.FG.ensure(nb * 2 * a, &grew) && w.Pm.ensure(nb * a, &grew);
  ok &= w.Yo.ensure(nb * a, &grew) && w.O.ensure(nb * a, &grew);
  ok &= w.skip.ensure(a, &grew) && w.Y1.ensure(a, &grew) && w.S2.ensure(a, &grew);
  ok &= w.col.ensure((size_t)w.KS * a, &grew) && w.dcol.ensure((size_t)w.KS * a, &grew);
  ok &= w.dz.ensure(a, &grew) && w.dskip.ensure(a, &grew) && w.dy.ensure(2 * a, &grew) && w.dp.ensure(a, &grew);
  if (!ok) return h->fail(NASR_ERR_HIP, "hipMalloc failed while sizing batch buffers");
  h->B = B; h->Bp = Bp; h->T = T; h->Lmax = Lmax; h->Tp = T; h->KS = KSa;
  return NASR_OK;
}

int wn_forward(nasr_ctx* h, bool training) {
  if (!h->resident) return h->fail(NASR_ERR_STATE, "no resident batch: call nasr_upload_batch first");
  WnState& w = *h->wn;
  const int D = w.D, KS = w.KS;
  const WnRows rw{h->T, h->B, h->Bp};
  const int R = rw.R();
  const size_t a = (size_t)R * D;
  const float* P = h->P;
  const float eps = w.eps;
  hipStream_t st = h->st;
  HIPCHK(h, hipMemsetAsync(h->Gbase, 0, GRAD_HEAD * 4, st));   // the step's fault word (nothing here raises it)
  // statistics of site s: the batch's (training) or the moving ones (inference)
  auto stats = [&](int s, const float* y, int nch, const float** mean, const float** var) {
    if (training) {
      launch_wn_bn_stats(y, nch, rw, w.bessel[s] != 0, w.bmean + (size_t)s * D, w.bvar + (size_t)s * D,
                         w.bvup + (size_t)s * D, w.ws, st);
      *mean = w.bmean + (size_t)s * D;
      *var = w.bvar + (size_t)s * D;
    } else {
      *mean = w.mm + (size_t)s * D;
      *var = w.mv + (size_t)s * D;
    }
  };
  const float *mean, *var;
  PhaseScope ps(h, PH_XPROJ);
  // front/conv_in: z0 = tanh(BN(X0 W))
  if (int rc = gemm_dense(h, h->X0.as<float>(), P + w.off_win, fp(w.Y0), R, D, h->Fp, h->Fp, D, D, false, false)) return rc;
  stats(0, fp(w.Y0), D, &mean, &var);
  launch_wn_bn_tanh(fp(w.Y0), mean, var, P + w.off_gamma[0], P + w.off_beta[0], eps, fp(w.Z), nullptr, nullptr, nullptr,
                    false, rw, D, st);
  for (int j = 0; j < w.nblk; ++j) {
    const float* z = fp(w.Z, j * a);
    float* yfg = fp(w.YFG, 2 * j * a);
    float* fg = fp(w.FG, 2 * j * a);
    float* pm = fp(w.Pm, j * a);
    float* yo = fp(w.Yo, j * a);
    // filter | gate: one GEMM of N = 2D over the K = KS*D (tap, channel) columns of the shifted rows
    launch_wn_im2col(z, fp(w.col), rw, D, KS, w.rate[j], st);
    if (int rc = gemm_dense(h, fp(w.col), P + w.off_wfg[j], yfg, R, 2 * D, KS * D, KS * D, 2 * D, 2 * D, false, false)) return rc;
    const int sf = w.site_filter(j);
    stats(sf, yfg, 2 * D, &mean, &var);
    launch_wn_bn_gate(yfg, mean, var, P + w.off_gamma[sf], P + w.off_beta[sf], eps, fg, pm, rw, D, st);
    // conv_out, residual and skip
    if (int rc = gemm_dense(h, pm, P + w.off_wo[j], yo, R, D, D, D, D, D, false, false)) return rc;
    const int so = w.site_out(j);
    stats(so, yo, D, &mean, &var);
    launch_wn_bn_tanh(yo, mean, var, P + w.off_gamma[so], P + w.off_beta[so], eps, fp(w.O, j * a), z, fp(w.Z, (j + 1) * a),
                      fp(w.skip), j == 0, rw, D, st);
  }
  if (w.nblk == 0) HIPCHK(h, hipMemsetAsync(w.skip.p, 0, a * 4, st));
  // logit/conv_1 and conv_2 (no BN, no bias)
  if (int rc = gemm_dense(h, fp(w.skip), P + w.off_w1, fp(w.Y1), R, D, D, D, D, D, false, false)) return rc;
  stats(w.S - 1, fp(w.Y1), D, &mean, &var);
  launch_wn_bn_tanh(fp(w.Y1), mean, var, P + w.off_gamma[w.S - 1], P + w.off_beta[w.S - 1], eps, fp(w.S2), nullptr, nullptr,
                    nullptr, false, rw, D, st);
  if (int rc = gemm_dense(h, fp(w.S2), P + w.off_w2, h->logits.as<float>(), R, h->Cp, D, D, h->Cp, h->Cp, false, false)) return rc;
  if (training) {
    w.have_stats = true;
    if (!w.hold) {
      w.count += 1;
      launch_wn_bn_update(w.mm, w.mv, w.biased, w.bmean, w.bvup, w.S * D, w.omd, w.count, st);
    }
  }
  HIPCHK(h, hipGetLastError());
  h->have_fwd = true;
  return NASR_OK;
}

int wn_backward(nasr_ctx* h) {
  WnState& w = *h->wn;
  if (!w.have_stats) return h->fail(NASR_ERR_STATE, "WaveNet backward pass without a training forward pass");
  const int D = w.D, KS = w.KS;
  const WnRows rw{h->T, h->B, h->Bp};
  const int R = rw.R();
  const size_t a = (size_t)R * D;
  const float* P = h->P;
  float* G = h->G;
  const float eps = w.eps;
  hipStream_t st = h->st;
  if (int rc = logit_grads(h)) return rc;
  PhaseScope ps(h, PH_WGRAD);
  // batch-norm backward of site s over y [R][nch] with dy (the gradient wrt its output, activation derivative applied)
  auto bn_bwd = [&](int s, const float* y, float* dy, int nch) {
    const float* mean = w.bmean + (size_t)s * D;
    const float* var = w.bvar + (size_t)s * D;
    launch_wn_bn_bwd_sums(y, dy, mean, var, eps, nch, rw, G + w.off_beta[s], G + w.off_gamma[s], w.ws, st);
    launch_wn_bn_bwd_apply(dy, y, mean, var, P + w.off_gamma[s], G + w.off_beta[s], G + w.off_gamma[s], eps, nch, rw, st);
  };
  const float* dlog = h->logits.as<float>();
  float* dy = fp(w.dy);
  // conv_2: dW2 = S2^T dlogits, dS2 = dlogits W2^T
  if (int rc = gemm_dense(h, fp(w.S2), dlog, G + w.off_w2, D, h->Cp, R, D, h->Cp, h->Cp, true, false)) return rc;
  if (int rc = gemm_dense(h, dlog, P + w.off_w2, fp(w.dp), R, D, h->Cp, h->Cp, h->Cp, D, false, true)) return rc;
  // conv_1
  launch_wn_dtanh(dy, fp(w.dp), nullptr, fp(w.S2), rw, D, st);
  bn_bwd(w.S - 1, fp(w.Y1), dy, D);
  if (int rc = gemm_dense(h, fp(w.skip), dy, G + w.off_w1, D, D, R, D, D, D, true, false)) return rc;
  if (int rc = gemm_dense(h, dy, P + w.off_w1, fp(w.dskip), R, D, D, D, D, D, false, true)) return rc;
  HIPCHK(h, hipMemsetAsync(w.dz.p, 0, a * 4, st));   // the last block's residual output feeds nothing
  for (int j = w.nblk - 1; j >= 0; --j) {
    const float* z = fp(w.Z, j * a);
    const float* yfg = fp(w.YFG, 2 * j * a);
    const float* pm = fp(w.Pm, j * a);
    // conv_out: its output went to the residual (dz) and to the skip sum (dskip)
    launch_wn_dtanh(dy, fp(w.dz), fp(w.dskip), fp(w.O, j * a), rw, D, st);
    bn_bwd(w.site_out(j), fp(w.Yo, j * a), dy, D);
    if (int rc = gemm_dense(h, pm, dy, G + w.off_wo[j], D, D, R, D, D, D, true, false)) return rc;
    if (int rc = gemm_dense(h, dy, P + w.off_wo[j], fp(w.dp), R, D, D, D, D, D, false, true)) return rc;
    // the gate, then batch norm of filter and gate together (2D channels)
    launch_wn_dgate(dy, fp(w.dp), fp(w.FG, 2 * j * a), rw, D, st);
    bn_bwd(w.site_filter(j), yfg, dy, 2 * D);
    launch_wn_im2col(z, fp(w.col), rw, D, KS, w.rate[j], st);
    if (int rc = gemm_dense(h, fp(w.col), dy, G + w.off_wfg[j], KS * D, 2 * D, R, KS * D, 2 * D, 2 * D, true, false)) return rc;
    // data gradient: the shifted-tap products, then each tap's rows moved back (the taps reversed) onto the residual's
    if (int rc = gemm_dense(h, dy, P + w.off_wfg[j], fp(w.dcol), R, KS * D, 2 * D, 2 * D, 2 * D, KS * D, false, true)) return rc;
    launch_wn_col2im_add(fp(w.dcol), fp(w.dz), rw, D, KS, w.rate[j], st);
  }
  // front/conv_in
  launch_wn_dtanh(dy, fp(w.dz), w.nblk == 0 ? fp(w.dskip) : nullptr, fp(w.Z), rw, D, st);
  bn_bwd(0, fp(w.Y0), dy, D);
  if (int rc = gemm_dense(h, h->X0.as<float>(), dy, G + w.off_win, h->Fp, D, R, h->Fp, D, D, true, false)) return rc;
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev_bucket.back(), st));   // one bucket: the whole gradient with the fault word
  h->have_grads = true;
  return NASR_OK;
}

}  // namespace nasr_impl

void nasr_impl::WnStateDelete::operator()(WnState* w) const { delete w; }

extern "C" {

int nasr_create_wavenet(const nasr_wavenet_cfg* cfg, int device_id, void* stream, nasr_handle* out) {
  if (!cfg || !out) {
    g_create_error = "nasr_create_wavenet: null argument";
    return NASR_ERR_ARG;
  }
  *out = nullptr;
  if (cfg->feature_size < 1 || cfg->num_classes < 2) {
    g_create_error = "nasr_create_wavenet: feature_size must be >= 1 and num_classes >= 2";
    return NASR_ERR_ARG;
  }
  if (cfg->dim != 128 || cfg->kernel_size != 7) {
    g_create_error = "nasr_create_wavenet: only dim = 128 and kernel_size = 7 (the reference's) are implemented";
    return NASR_ERR_ARG;
  }
  if (cfg->num_blocks < 0 || cfg->num_rates < 0 || cfg->num_rates > 8 || cfg->num_blocks * cfg->num_rates > 64) {
    g_create_error = "nasr_create_wavenet: num_rates must be in [0,8] and num_blocks * num_rates <= 64";
    return NASR_ERR_ARG;
  }
  for (int i = 0; i < cfg->num_rates; ++i)
    if (cfg->rates[i] < 1) {
      g_create_error = "nasr_create_wavenet: rates must be >= 1";
      return NASR_ERR_ARG;
    }
  if (!(cfg->bn_epsilon > 0.f) || !(cfg->bn_decay >= 0.f && cfg->bn_decay < 1.f)) {
    g_create_error = "nasr_create_wavenet: bn_epsilon must be > 0 and bn_decay in [0,1)";
    return NASR_ERR_ARG;
  }
  nasr_ctx* h = nullptr;
  if (int rc = handle_open("nasr_create_wavenet", Family::WaveNet, device_id, stream, &h, nullptr)) return rc;
  h->beta1 = cfg->beta1; h->beta2 = cfg->beta2; h->epsilon = cfg->epsilon;
  h->lr = cfg->learning_rate;
  h->graph_mode = false;
  h->wn.reset(new WnState());
  WnState& w = *h->wn;
  w.cfg = *cfg;
  w.D = cfg->dim; w.KS = cfg->kernel_size;
  w.nblk = cfg->num_blocks * cfg->num_rates;
  for (int i = 0; i < cfg->num_blocks; ++i)
    for (int r = 0; r < cfg->num_rates; ++r) w.rate.push_back(cfg->rates[r]);
  w.eps = cfg->bn_epsilon;
  w.omd = (float)(1.0 - (double)cfg->bn_decay);
  wn_layout(h);
  const size_t sb = (size_t)w.S * w.D * 4;
  if (!alloc_param_buffers(h)) return create_fail(h, NASR_ERR_HIP, "hipMalloc of parameter buffers failed");
  if (hipMalloc(w.mm.out(), sb) != hipSuccess || hipMalloc(w.mv.out(), sb) != hipSuccess ||
      hipMalloc(w.biased.out(), sb) != hipSuccess || hipMalloc(w.bmean.out(), sb) != hipSuccess ||
      hipMalloc(w.bvar.out(), sb) != hipSuccess || hipMalloc(w.bvup.out(), sb) != hipSuccess ||
      hipMalloc(w.ws.out(), (size_t)WN_STAT_WS * 4) != hipSuccess)
    return create_fail(h, NASR_ERR_HIP, "hipMalloc of the batch-norm state failed");
  // moving mean 0, moving variance 1 (contrib batch_norm's initialisers), zero-debias accumulator 0
  (void)hipMemsetAsync(w.mm, 0, sb, h->st);
  (void)hipMemsetAsync(w.biased, 0, sb, h->st);
  launch_fill(w.mv, 1.f, w.S * w.D, h->st);
  h->buckets.push_back({0, GRAD_HEAD + h->np_int});   // one bucket: the whole gradient, complete at the end of the backward pass
  if (int rc = handle_finish(h)) return rc;
  *out = h;
  return NASR_OK;
}

int64_t nasr_wavenet_bn_count(nasr_handle h) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  return (int64_t)w->S * w->D;
}

int nasr_wavenet_get_bn_state(nasr_handle h, float* moving_mean, float* moving_var, float* biased, int64_t n,
                              int64_t* updates) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  if (n != (int64_t)w->S * w->D) return h->fail(NASR_ERR_ARG, "nasr_wavenet_get_bn_state: wrong length");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t sb = (size_t)n * 4;
  if (moving_mean) HIPCHK(h, hipMemcpyAsync(moving_mean, w->mm, sb, hipMemcpyDeviceToHost, h->st));
  if (moving_var) HIPCHK(h, hipMemcpyAsync(moving_var, w->mv, sb, hipMemcpyDeviceToHost, h->st));
  if (biased) HIPCHK(h, hipMemcpyAsync(biased, w->biased, sb, hipMemcpyDeviceToHost, h->st));
  if (updates) *updates = w->count;
  HIPCHK(h, hipStreamSynchronize(h->st));
  return NASR_OK;
}

int nasr_wavenet_set_bn_state(nasr_handle h, const float* moving_mean, const float* moving_var, const float* biased,
                              int64_t n, int64_t updates) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  if (n != (int64_t)w->S * w->D || updates < 0 || !moving_mean || !moving_var || !biased)
    return h->fail(NASR_ERR_ARG, "nasr_wavenet_set_bn_state: wrong length, null array or negative update count");
  HIPCHK(h, hipSetDevice(h->device));
  const size_t sb = (size_t)n * 4;
  HIPCHK(h, hipMemcpyAsync(w->mm, moving_mean, sb, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(w->mv, moving_var, sb, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(w->biased, biased, sb, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  w->count = updates;
  return NASR_OK;
}

int nasr_wavenet_set_bn_hold(nasr_handle h, int hold) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  w->hold = hold != 0;
  return NASR_OK;
}

int nasr_wavenet_get_batch_stats(nasr_handle h, float* mean, float* var, int64_t n) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  if (n != (int64_t)w->S * w->D || !mean || !var) return h->fail(NASR_ERR_ARG, "nasr_wavenet_get_batch_stats: wrong length");
  if (!w->have_stats) return h->fail(NASR_ERR_STATE, "nasr_wavenet_get_batch_stats: no training pass has run");
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipMemcpyAsync(mean, w->bmean, (size_t)n * 4, hipMemcpyDeviceToHost, h->st));
  HIPCHK(h, hipMemcpyAsync(var, w->bvup, (size_t)n * 4, hipMemcpyDeviceToHost, h->st));
  return sync_checked(h);
}

int nasr_wavenet_apply_bn_stats(nasr_handle h, const float* mean, const float* var, int64_t n, int count) {
  WAVENET_CALL(h);
  WnState* w = h->wn.get();
  if (n != (int64_t)w->S * w->D || count < 0 || (count > 0 && (!mean || !var)))
    return h->fail(NASR_ERR_ARG, "nasr_wavenet_apply_bn_stats: wrong length or count");
  if (count == 0) return NASR_OK;
  HIPCHK(h, hipSetDevice(h->device));
  DevPtr<float> tmp;
  const size_t sb = (size_t)n * count * 4;
  HIPCHK(h, hipMalloc(tmp.out(), 2 * sb));
  HIPCHK(h, hipMemcpyAsync(tmp, mean, sb, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipMemcpyAsync(tmp + (size_t)n * count, var, sb, hipMemcpyHostToDevice, h->st));
  for (int i = 0; i < count; ++i) {
    w->count += 1;
    launch_wn_bn_update(w->mm, w->mv, w->biased, tmp + (size_t)i * n, tmp + (size_t)(count + i) * n, (int)n, w->omd, w->count,
                        h->st);
  }
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipStreamSynchronize(h->st));   // (before tmp is freed)
  return NASR_OK;
}

}  // extern "C"
