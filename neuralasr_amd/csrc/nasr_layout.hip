// nasr_layout.hip — parameter layout of a handle (TF variable order <-> the padded internal buffers), the operand images the
// kernels keep of the weights (repack; the recurrent matrices' images are nasr_rec.hip's), host <-> device parameter
// copies.  See include/nasr.h and DESIGN.md §3.
#include "nasr_lstm.h"

using namespace nasr;
using namespace nasr_impl;

namespace nasr_impl {

std::string g_create_error;
thread_local std::string t_err;
thread_local const void* t_err_handle = nullptr;

// scales of src [rows][K]: per row into `row`, per column into `col` (either may be NULL)
void pl_scales(nasr_ctx* h, const float* src, int rows, int K, int ld, SV* row, SV* col, hipStream_t st) {
  launch_tph_scales(src, rows, K, ld, row ? row->sp() : nullptr, row ? row->ip() : nullptr, col ? col->sp() : nullptr,
                    col ? col->ip() : nullptr, h->lstm->scws.as<float>(), st);
}
// planes of src [rows][K] (tpN, scaled per row by rs[]) and / or of its transpose (tpT, scaled per src column by cs[]);
// colpart: 64-row partial column sums for launch_colsum_parts
void pl_split(const float* src, unsigned char* tpN, unsigned char* tpT, int rows, int K, int ld, const float* rs,
              const float* cs, float* colpart, hipStream_t st) {
  launch_tph_split2(src, tpN, tpT, rows, K, ld, rs, 1.f, cs, 1.f, colpart, st);
}
// a_inv / b_inv: inverse scales of A's / B's rows; the strides apply to batch 1 of a two-batch launch
void pl_gemm(GemmTPHDesc g, const float* a_inv, const float* b_inv, hipStream_t st, int64_t ainv_bstride, int64_t binv_bstride) {
  g.a_inv = a_inv; g.b_inv = b_inv; g.ainv_bstride = ainv_bstride; g.binv_bstride = binv_bstride;
  launch_gemm_tph(g, st);
}
// A word in host-mapped pinned memory, written by a one-thread kernel in stream order (system-scope store): the host
// learns that everything enqueued before it has happened by READING MEMORY - no runtime call, no event.  (Waiting on a HIP
// event recorded a whole step earlier cost 0.4-0.75 ms per call here although the event had long fired.)
__global__ void stamp_kernel(unsigned* dst, unsigned value, float* f0_dst, const float* f0_src) {
  if (f0_dst) __hip_atomic_store(f0_dst, *f0_src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(dst, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_stamp(unsigned* dst, unsigned value, float* f0_dst, const float* f0_src, hipStream_t st) {
  hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, st, dst, value, f0_dst, f0_src);
}

// The values a step returns to the host (loss, fault word, greedy decode), written by ONE kernel straight into the host's
// pinned result buffer and stamped behind them - instead of four small device-to-host copies and a stamp launch per step.
// host: [loss f32][fault f32][lens i32 x Bp][ids i32 x n_ids]
__global__ __launch_bounds__(256) void publish_results_kernel(const float* __restrict__ loss, const float* __restrict__ fault,
                                                              const int* __restrict__ lens, int Bp, const int* __restrict__ ids,
                                                              int n_ids, unsigned* host, unsigned* stamp, unsigned value) {
  if (threadIdx.x == 0) {
    host[0] = __float_as_uint(*loss);
    host[1] = __float_as_uint(*fault);
  }
  for (int i = threadIdx.x; i < Bp; i += 256) host[2 + i] = (unsigned)lens[i];
  for (int i = threadIdx.x; i < n_ids; i += 256) host[2 + Bp + i] = (unsigned)ids[i];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(stamp, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
void launch_publish_results(const float* loss, const float* fault, const int* lens, int Bp, const int* ids, int n_ids, void* host,
                            unsigned* stamp, unsigned value, hipStream_t st) {
  hipLaunchKernelGGL(publish_results_kernel, dim3(1), dim3(256), 0, st, loss, fault, lens, Bp, ids, n_ids,
                     static_cast<unsigned*>(host), stamp, value);
}

bool wait_stamp(const uint32_t* w, uint32_t want, double timeout_s) {
  const volatile uint32_t* v = w;
  for (int i = 0; i < 4000; ++i)
    if (*v == want) return true;
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned n = 0;; ++n) {
    if (*v == want) return true;
    if ((n & 63) == 63) {
      if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return false;
      usleep(20);
    } else {
      sched_yield();
    }
  }
}

int sync_checked(nasr_ctx* h) {
  HIPCHK(h, hipStreamSynchronize(h->st));
  return rec_check(h);
}

hipEvent_t next_event(nasr_ctx* h) {
  if (h->ev_used == h->ev_pool.size()) (void)hipEventCreate(h->ev_pool.emplace_back().out());
  return h->ev_pool[h->ev_used++];
}
// ---- model layout ---------------------------------------------------------------------------
int build_layout(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  const nasr_model_cfg& c = ls->cfg;
  h->F = c.feature_size;
  ls->H = c.hidden;
  ls->L = c.num_layers;
  ls->D = c.bidirectional ? 2 : 1;
  h->C = c.num_classes;
  h->Fp = rup(h->F, 32);
  ls->Hp = rup(ls->H, 64);
  ls->N4 = 4 * ls->Hp;
  h->Cp = rup(h->C, 32);
  const bool concat = c.bidirectional && c.merge == NASR_MERGE_CONCAT;
  const int D = ls->D, Hp = ls->Hp, N4 = ls->N4, H = ls->H;
  const int lstm_out = concat ? 2 * H : H, lstm_outp = concat ? 2 * Hp : Hp;

  // dense stages
  ls->npre = c.num_pre;
  ls->has_post = c.post_width > 0;
  ls->ndense = ls->npre + (ls->has_post ? 1 : 0);
  ls->dWid.assign(ls->ndense, 0); ls->dWp.assign(ls->ndense, 0); ls->dIn.assign(ls->ndense, 0); ls->dIp.assign(ls->ndense, 0);
  for (int i = 0; i < ls->npre; ++i) {
    ls->dWid[i] = c.pre_width[i]; ls->dWp[i] = rup(c.pre_width[i], 64);
    ls->dIn[i] = i == 0 ? h->F : ls->dWid[i - 1];
    ls->dIp[i] = i == 0 ? h->Fp : ls->dWp[i - 1];
  }
  if (ls->has_post) {
    const int i = ls->npre;
    ls->dWid[i] = c.post_width; ls->dWp[i] = rup(c.post_width, 64);
    ls->dIn[i] = lstm_out; ls->dIp[i] = lstm_outp;
  }
  ls->F0 = ls->npre ? ls->dWid[ls->npre - 1] : h->F;
  ls->Pin = ls->has_post ? c.post_width : lstm_out;
  ls->Pinp = ls->has_post ? ls->dWp[ls->npre] : lstm_outp;

  int64_t off = 0;
  ls->off_dw.assign(ls->ndense, 0); ls->off_db.assign(ls->ndense, 0);
  for (int i = 0; i < ls->ndense; ++i) {
    ls->off_dw[i] = off; off += (int64_t)ls->dIp[i] * ls->dWp[i];
    ls->off_db[i] = off; off += ls->dWp[i];
  }
  ls->Ip.resize(ls->L);
  ls->off_wx.resize(ls->L);
  ls->off_bias.resize(ls->L);
  ls->off_u.resize((size_t)ls->L * D);
  for (int l = 0; l < ls->L; ++l) {
    ls->Ip[l] = l == 0 ? (ls->npre ? ls->dWp[ls->npre - 1] : h->Fp) : D * Hp;
    ls->off_wx[l] = off;
    off += (int64_t)ls->Ip[l] * D * N4;
    ls->off_bias[l] = off;
    off += (int64_t)D * N4;
    for (int d = 0; d < D; ++d) {
      ls->off_u[(size_t)l * D + d] = off;
      off += (int64_t)Hp * N4;
    }
  }
  ls->off_w = off;
  off += (int64_t)ls->Pinp * h->Cp;
  ls->off_b = off;
  off += h->Cp;
  h->np_int = off;  // every term is a multiple of 32
  if (off >= (int64_t)1 << 31) return h->fail(NASR_ERR_ARG, "model too large for 32-bit parameter indexing");

  // TF variable order + element map.  Plain (Bi)LstmCTCNet: cells, W, b.  DeepSpeech family (creation order of
  // networks/deepspeech.py): b1,h1,b2,h2,b3,h3, cells, b5,h5, b6,h6.
  const bool ds = ls->ndense > 0;
  h->tensors.clear();
  int64_t tfo = 0;
  auto add = [&](const std::string& n, int64_t r, int64_t cc) {
    h->tensors.push_back({n, tfo, r, cc});
    tfo += r * cc;
  };
  for (int i = 0; i < ls->npre; ++i) {
    add("b" + std::to_string(i + 1), ls->dWid[i], 1);
    add("h" + std::to_string(i + 1), ls->dIn[i], ls->dWid[i]);
  }
  for (int l = 0; l < ls->L; ++l) {
    const int I = l == 0 ? ls->F0 : D * H;
    for (int d = 0; d < D; ++d) {
      std::string pre = "l" + std::to_string(l) + "/";
      if (D == 2) pre += d == 0 ? "fw/" : "bw/";
      add(pre + "kernel", I + H, 4 * H);
      add(pre + "bias", 4 * H, 1);
    }
  }
  if (ds) {
    if (ls->has_post) {
      add("b5", ls->dWid[ls->npre], 1);
      add("h5", ls->dIn[ls->npre], ls->dWid[ls->npre]);
    }
    add("b6", h->C, 1);
    add("h6", ls->Pin, h->C);
  } else {
    add("W", ls->Pin, h->C);
    add("b", h->C, 1);
  }
  h->np_tf = tfo;
  h->tf2int.assign((size_t)tfo, 0);
  size_t ti = 0;
  // rows of a matrix fed by the concatenated (fw, bw) outputs: the bw half starts at the padded width
  auto cat_row = [&](int r) { return (D == 2 && concat && r >= H) ? Hp + (r - H) : r; };
  auto map_dense = [&](int i, bool from_lstm) {
    const TensorInfo& tb = h->tensors[ti++];
    for (int cc = 0; cc < ls->dWid[i]; ++cc) h->tf2int[(size_t)(tb.offset + cc)] = (int32_t)(ls->off_db[i] + cc);
    const TensorInfo& tw = h->tensors[ti++];
    for (int r = 0; r < ls->dIn[i]; ++r) {
      const int ir = from_lstm ? cat_row(r) : r;
      for (int cc = 0; cc < ls->dWid[i]; ++cc)
        h->tf2int[(size_t)(tw.offset + (int64_t)r * ls->dWid[i] + cc)] = (int32_t)(ls->off_dw[i] + (int64_t)ir * ls->dWp[i] + cc);
    }
  };
  for (int i = 0; i < ls->npre; ++i) map_dense(i, false);
  for (int l = 0; l < ls->L; ++l) {
    const int I = l == 0 ? ls->F0 : D * H;
    for (int d = 0; d < D; ++d) {
      const TensorInfo& tk = h->tensors[ti++];
      for (int r = 0; r < I + H; ++r) {
        for (int cc = 0; cc < 4 * H; ++cc) {
          const int g = cc / H, j = cc % H;
          int64_t dst;
          if (r < I) {
            int ir = r;
            if (l > 0 && D == 2 && r >= H) ir = Hp + (r - H);
            dst = ls->off_wx[l] + (int64_t)ir * D * N4 + d * N4 + 4 * j + g;
          } else {
            dst = ls->off_u[(size_t)l * D + d] + (int64_t)(r - I) * N4 + 4 * j + g;
          }
          h->tf2int[(size_t)(tk.offset + (int64_t)r * 4 * H + cc)] = (int32_t)dst;
        }
      }
      const TensorInfo& tb = h->tensors[ti++];
      for (int cc = 0; cc < 4 * H; ++cc) {
        const int g = cc / H, j = cc % H;
        h->tf2int[(size_t)(tb.offset + cc)] = (int32_t)(ls->off_bias[l] + d * N4 + 4 * j + g);
      }
    }
  }
  if (ls->has_post) map_dense(ls->npre, true);
  auto map_w = [&]() {
    const TensorInfo& tw = h->tensors[ti++];
    for (int r = 0; r < ls->Pin; ++r) {
      const int ir = ls->has_post ? r : cat_row(r);
      for (int cc = 0; cc < h->C; ++cc)
        h->tf2int[(size_t)(tw.offset + (int64_t)r * h->C + cc)] = (int32_t)(ls->off_w + (int64_t)ir * h->Cp + cc);
    }
  };
  auto map_b = [&]() {
    const TensorInfo& tb = h->tensors[ti++];
    for (int cc = 0; cc < h->C; ++cc) h->tf2int[(size_t)(tb.offset + cc)] = (int32_t)(ls->off_b + cc);
  };
  if (ds) { map_b(); map_w(); } else { map_w(); map_b(); }
  return NASR_OK;
}

int repack(nasr_ctx* h) {
  LstmState* const ls = h->lstm.get();
  if (!ls) return NASR_OK;   // the WaveNet's and LAS's GEMMs read the fp32 parameters directly: no operand images
  ls->repack_seq += 1;
  // only the operand images of the kernels in use (a switch of the recurrence's kind calls repack again)
  // scales of every matrix that needs them - recurrent matrices of the persistent / wide kernels, input and dense
  // weights of the plane GEMMs - in ONE batch (two launches), then the images
  std::vector<TphScaleJob> jobs = rec_scale_jobs(h);
  for (int l = 0; l < ls->L; ++l) {
    const bool back = l > 0 || ls->npre > 0;
    jobs.push_back({h->P + ls->off_wx[l], ls->Ip[l], ls->D * ls->N4, ls->D * ls->N4, back ? ls->sc_wr[l].sp() : nullptr,
                    back ? ls->sc_wr[l].ip() : nullptr, ls->sc_wc[l].sp(), ls->sc_wc[l].ip()});
  }
  for (int i = 0; i < ls->ndense; ++i) {
    const bool back = i > 0 || ls->npre == 0;
    jobs.push_back({h->P + ls->off_dw[i], ls->dIp[i], ls->dWp[i], ls->dWp[i], back ? ls->sc_dr[i].sp() : nullptr,
                    back ? ls->sc_dr[i].ip() : nullptr, ls->sc_dc[i].sp(), ls->sc_dc[i].ip()});
  }
  {
    bool g2 = false;
    if (!ls->scws.ensure(tph_scale_batch_ws_floats(jobs.data(), (int)jobs.size()) * 4, &g2))
      return h->fail(NASR_ERR_HIP, "allocation of the scale workspace failed");
  }
  launch_tph_scales_batch(jobs.data(), (int)jobs.size(), ls->scws.as<float>(), h->st);
  rec_images(h);
  for (int l = 0; l < ls->L; ++l) {
    // forward operand = planes of Wx^T, input-gradient operand = planes of Wx: one pass where both are needed
    const bool back = l > 0 || ls->npre > 0;
    const float* W = h->P + ls->off_wx[l];
    pl_split(W, back ? ls->WbTP + ls->off_wbtp[l] : nullptr, ls->WfTP + ls->off_wftp[l], ls->Ip[l], ls->D * ls->N4,
             ls->D * ls->N4, back ? ls->sc_wr[l].sp() : nullptr, ls->sc_wc[l].sp(), nullptr, h->st);
  }
  for (int i = 0; i < ls->ndense; ++i) {
    const bool back = i > 0 || ls->npre == 0;   // the first pre stage reads the features: no gradient wrt its input
    const float* W = h->P + ls->off_dw[i];
    pl_split(W, back ? ls->DbTP + ls->off_dbtp[i] : nullptr, ls->DfTP + ls->off_dftp[i], ls->dIp[i], ls->dWp[i], ls->dWp[i],
             back ? ls->sc_dr[i].sp() : nullptr, ls->sc_dc[i].sp(), nullptr, h->st);
  }
  HIPCHK(h, hipGetLastError());
  return NASR_OK;
}

int scatter_to_device(nasr_ctx* h, const float* tf_flat, float* dev) {
  std::vector<float> host((size_t)h->np_int, 0.f);
  for (int64_t i = 0; i < h->np_tf; ++i) host[(size_t)h->tf2int[(size_t)i]] = tf_flat[i];
  HIPCHK(h, hipMemcpyAsync(dev, host.data(), (size_t)h->np_int * 4, hipMemcpyHostToDevice, h->st));
  HIPCHK(h, hipStreamSynchronize(h->st));
  return NASR_OK;
}

int gather_from_device(nasr_ctx* h, const float* dev, float* tf_flat) {
  std::vector<float> host((size_t)h->np_int);
  HIPCHK(h, hipMemcpyAsync(host.data(), dev, (size_t)h->np_int * 4, hipMemcpyDeviceToHost, h->st));
  if (int rc = sync_checked(h)) return rc;
  for (int64_t i = 0; i < h->np_tf; ++i) tf_flat[i] = host[(size_t)h->tf2int[(size_t)i]];
  return NASR_OK;
}

// ---- batch buffers --------------------------------------------------------------------------
}  // namespace nasr_impl
