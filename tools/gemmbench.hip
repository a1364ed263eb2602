// gemmbench.hip — times the GEMM shapes of the training step (B 16, T 500, H 500, F 546).
// hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/gemmbench.hip -o tools/sb_gemm -ldl
//
// `sb_gemm --ab [reps] name=lib.so ...`: the plane GEMM (gemm_tph.hip) of this tree against other builds of it, ALTERNATING
// in one process on one device - the only way two kernels compare (devices differ by up to 12 % on MFMA-dense loops).
// A build to compare against is this file compiled as a library around another copy of gemm_tph.hip, e.g. the parent's:
//   git show HEAD~1:neuralasr_amd/csrc/gemm_tph.hip > /tmp/parent/gemm_tph.hip
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wl,-Bsymbolic -DGEMMBENCH_LIB \
//         -DGEMM_TPH_SRC='"/tmp/parent/gemm_tph.hip"' -Ineuralasr_amd/csrc tools/gemmbench.hip -o tools/sb_gemm_parent.so
//   tools/sb_gemm --ab 5 parent=tools/sb_gemm_parent.so
// Shapes: the flagship step's (xproj, dx, dWx, the two-direction dU with its shifts, the side form of the weight gradients)
// and DeepSpeech's (B 32, 2048 wide); operand planes hold random halves of the magnitudes real planes have.
#ifndef GEMM_TPH_SRC
#define GEMM_TPH_SRC "../neuralasr_amd/csrc/gemm_tph.hip"
#endif
#ifdef GEMMBENCH_LIB
#include GEMM_TPH_SRC
#include "../neuralasr_amd/csrc/optim.hip"
extern "C" int gb_prepare() { return (int)nasr::gemm_tph_prepare(); }
extern "C" void gb_launch(const nasr::GemmTPHDesc* g, hipStream_t st) { nasr::launch_gemm_tph(*g, st); }
#else
#include "../neuralasr_amd/csrc/gemm.hip"
#include GEMM_TPH_SRC
#include "../neuralasr_amd/csrc/optim.hip"
#include <dlfcn.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
using namespace nasr;
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)
static float* dev_rand(size_t n) {
  std::vector<float> h(n);
  for (auto& v : h) v = rand() / (float)RAND_MAX - 0.5f;
  float* d; CK(hipMalloc(&d, n * 4)); CK(hipMemcpy(d, h.data(), n * 4, hipMemcpyHostToDevice));
  return d;
}

// ---- --ab: this tree's launch_gemm_tph and the libraries' gb_launch, alternating
// plane halves: part 0 tiles uniform in +-2^15 (a row's maximum lands in [2^14, 2^15)), part 1 tiles 2^-11 of that
__global__ void fill_planes_kernel(_Float16* p, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned x = (unsigned)i * 2654435761u ^ (unsigned)(i >> 32) * 40503u;
    x ^= x >> 15; x *= 2246822519u; x ^= x >> 13; x *= 3266489917u; x ^= x >> 16;
    const float u = (int)(x & 0xffff) - 32768;
    p[i] = (_Float16)(((i >> 9) & 1) ? u * (1.f / 2048.f) : u * 0.999f);
  }
}
static void gb_local(const GemmTPHDesc* g, hipStream_t st) { launch_gemm_tph(*g, st); }
static int run_ab(int argc, char** argv) {
  typedef void (*launch_fn)(const GemmTPHDesc*, hipStream_t);
  struct Impl { std::string name; launch_fn launch; };
  std::vector<Impl> impls = {{"tree", gb_local}};
  int reps = 5;
  for (int i = 2; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) { reps = atoi(argv[i]); continue; }
    void* so = dlopen(eq + 1, RTLD_NOW | RTLD_LOCAL);
    if (!so) { printf("%s\n", dlerror()); return 1; }
    auto prep = (int (*)())dlsym(so, "gb_prepare");
    auto fn = (launch_fn)dlsym(so, "gb_launch");
    if (!prep || !fn || prep() != 0) { printf("%s: no gb_prepare / gb_launch\n", eq + 1); return 1; }
    impls.push_back({std::string(argv[i], eq - argv[i]), fn});
  }
  CK(gemm_tph_prepare());
  struct Case { const char* name; int M, N, K, nbatch, side; };
  const Case cases[] = {
      {"xproj 8000x4096x576", 8000, 4096, 576, 1, 0},       {"xproj 8000x4096x1024", 8000, 4096, 1024, 1, 0},
      {"dx 8000x1024x4096", 8000, 1024, 4096, 1, 0},        {"dWx 1024x4096x8000", 1024, 4096, 8000, 1, 0},
      {"dWx 576x4096x8000", 576, 4096, 8000, 1, 0},         {"dU 2x512x2048x8000", 512, 2048, 8000, 2, 0},
      {"side dWx 1024x4096x8000", 1024, 4096, 8000, 1, 1},  {"side dU 2x512x2048x8000", 512, 2048, 8000, 2, 1},
      {"ds xproj 16000x16384x2048", 16000, 16384, 2048, 1, 0}, {"ds dx 16000x2048x16384", 16000, 2048, 16384, 1, 0},
      {"ds dWx 2048x16384x16000", 2048, 16384, 16000, 1, 0},   {"ds dU 2x2048x8192x16000", 2048, 8192, 16000, 2, 0},
  };
  const size_t plane_bytes = tph_bytes(16384, 16384), c_floats = (size_t)16000 * 16384, slab_floats = (size_t)1 << 28;
  unsigned char *PA, *PB;
  float *C, *slabs, *ones;
  CK(hipMalloc(&PA, plane_bytes)); CK(hipMalloc(&PB, plane_bytes)); CK(hipMalloc(&C, c_floats * 4)); CK(hipMalloc(&slabs, slab_floats * 4));
  CK(hipMalloc(&ones, 16384 * 4));
  hipStream_t st; CK(hipStreamCreate(&st));
  hipLaunchKernelGGL(fill_planes_kernel, dim3(4096), dim3(256), 0, st, (_Float16*)PA, plane_bytes / 2);
  hipLaunchKernelGGL(fill_planes_kernel, dim3(4096), dim3(256), 0, st, (_Float16*)PB + 512, plane_bytes / 2 - 512);
  launch_fill(ones, 1.f, 16384, st);
  CK(hipStreamSynchronize(st)); CK(hipGetLastError());
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  const int nl = 10;
  const char* only = getenv("GEMMBENCH_ONLY");         // substring of the case names to run
  for (const Case& c : cases) {
    if (only && !strstr(c.name, only)) continue;
    GemmTPHDesc g{};
    const int nkb = (c.K + 15) / 16;
    g.A = PA; g.B = PB; g.C = C; g.M = c.M; g.N = c.N; g.K = c.K; g.nkbA = nkb; g.nkbB = nkb; g.ldc = c.N;
    g.a_inv = ones; g.b_inv = ones; g.side = c.side != 0; g.nbatch = c.nbatch;
    if (c.nbatch == 2) {
      g.a_kshift = -16; g.a_kshift1 = 16;
      g.a_bstride = (size_t)(c.M / 32) * nkb * 2048; g.b_bstride = (size_t)(c.N / 32) * nkb * 2048;
      g.c_bstride = (int64_t)c.M * c.N; g.ainv_bstride = c.M; g.binv_bstride = c.N;
    }
    g.split_k = gemm_tph_pick_split(c.M, c.N, c.K, c.nbatch); g.slabs = slabs;
    if ((size_t)g.split_k * c.nbatch * c.M * c.N > slab_floats) { printf("%s: slabs too small\n", c.name); continue; }
    std::vector<std::vector<float>> us(impls.size());
    std::vector<float> first;
    for (int i = 0; i < 2 * nl; ++i)           // clocks settle on the shape before anything is timed
      for (auto& im : impls) im.launch(&g, st);
    for (int r = 0; r < reps; ++r)
      for (size_t k = 0; k < impls.size(); ++k) {
        for (int i = 0; i < 2; ++i) impls[k].launch(&g, st);
        CK(hipEventRecord(a, st));
        for (int i = 0; i < nl; ++i) impls[k].launch(&g, st);
        CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b)); CK(hipGetLastError());
        float ms; CK(hipEventElapsedTime(&ms, a, b));
        us[k].push_back(ms * 1000.f / nl);
        if (r == 0) {          // every build must give the same bits
          std::vector<float> h((size_t)c.nbatch * c.M * c.N);
          CK(hipMemcpy(h.data(), C, h.size() * 4, hipMemcpyDeviceToHost));
          if (k == 0) first = h;
          else if (memcmp(first.data(), h.data(), h.size() * 4) != 0) printf("%s: %s DIFFERS from %s\n", c.name, impls[k].name.c_str(), impls[0].name.c_str());
        }
      }
    for (size_t k = 0; k < impls.size(); ++k) {
      const float lo = *std::min_element(us[k].begin(), us[k].end()), hi = *std::max_element(us[k].begin(), us[k].end());
      printf("%-26s split %2d  %-8s us/launch min %8.1f max %8.1f  %6.1f TF-equiv  runs:", c.name, g.split_k, impls[k].name.c_str(), lo, hi,
             2.0 * c.nbatch * c.M * c.N * c.K / lo / 1e6);
      for (float v : us[k]) printf(" %.1f", v);
      printf("\n");
    }
    fflush(stdout);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--ab")) return run_ab(argc, argv);
  const int R = 8000;
  float* X = dev_rand((size_t)R * 1024);
  float* G = dev_rand((size_t)R * 4096);
  float* W = dev_rand((size_t)1024 * 4096);
  float* O = dev_rand((size_t)R * 4096);
  float* bias = dev_rand(4096);
  float* slabs; CK(hipMalloc(&slabs, (size_t)8 * 1024 * 4096 * 4));
  hipStream_t st; CK(hipStreamCreate(&st));
  struct Case { const char* name; GemmDesc g; };
  std::vector<Case> cases;
  { GemmDesc g{}; g.A = X; g.B = W; g.C = O; g.M = R; g.N = 4096; g.K = 576; g.lda = 576; g.ldb = 4096; g.ldc = 4096; g.a_rows = R; g.bias = bias; g.split_k = 1; cases.push_back({"xproj  NN 8000x4096x576 ", g}); }
  { GemmDesc g{}; g.A = X; g.B = W; g.C = O; g.M = R; g.N = 4096; g.K = 1024; g.lda = 1024; g.ldb = 4096; g.ldc = 4096; g.a_rows = R; g.bias = bias; g.split_k = 1; cases.push_back({"xproj  NN 8000x4096x1024", g}); }
  { GemmDesc g{}; g.A = X; g.B = G; g.C = O; g.M = 576; g.N = 4096; g.K = R; g.lda = 576; g.ldb = 4096; g.ldc = 4096; g.a_col = true; g.a_rows = R; g.split_k = gemm_pick_split(576, 4096, R); g.slabs = slabs; cases.push_back({"dWx    TN 576x4096x8000 ", g}); }
  { GemmDesc g{}; g.A = X; g.B = G; g.C = O; g.M = 1024; g.N = 4096; g.K = R; g.lda = 1024; g.ldb = 4096; g.ldc = 4096; g.a_col = true; g.a_rows = R; g.split_k = gemm_pick_split(1024, 4096, R); g.slabs = slabs; cases.push_back({"dWx    TN 1024x4096x8000", g}); }
  { GemmDesc g{}; g.A = X; g.B = G; g.C = O; g.M = 512; g.N = 2048; g.K = R; g.lda = 1024; g.ldb = 4096; g.ldc = 2048; g.a_col = true; g.a_shift = -16; g.a_rows = R; g.split_k = gemm_pick_split(512, 2048, R); g.slabs = slabs; cases.push_back({"dU     TN 512x2048x8000 ", g}); }
  { GemmDesc g{}; g.A = G; g.B = W; g.C = O; g.M = R; g.N = 1024; g.K = 4096; g.lda = 4096; g.ldb = 4096; g.ldc = 1024; g.b_col = true; g.a_rows = R; g.split_k = 1; cases.push_back({"dX     NT 8000x1024x4096", g}); }
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  for (auto& c : cases) {
    for (int i = 0; i < 3; ++i) launch_gemm(c.g, st);
    CK(hipStreamSynchronize(st));
    float best = 1e9f;
    for (int i = 0; i < 10; ++i) {
      CK(hipEventRecord(a, st)); launch_gemm(c.g, st); CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b));
      float ms; CK(hipEventElapsedTime(&ms, a, b)); best = ms < best ? ms : best;
    }
    double fl = 2.0 * c.g.M * c.g.N * c.g.K;
    printf("%s split %d : %.3f ms  %.1f TF\n", c.name, c.g.split_k, best, fl / best / 1e9);
  }
  // ---- the shapes of the step in NT form (A [M][K], B [N][K]): operands are views of the buffers above
  struct NT { const char* name; int M, N, K, split; const float* A; size_t a_elems; const float* B; size_t b_elems; };
  const size_t nX = (size_t)R * 1024, nG = (size_t)R * 4096, nW = (size_t)1024 * 4096;
  std::vector<NT> nts = {{"xproj  NT 8000x4096x576 ", R, 4096, 576, 1, X, nX, W, nW}, {"xproj  NT 8000x4096x1024", R, 4096, 1024, 1, X, nX, W, nW},
                         {"dX     NT 8000x1024x4096", R, 1024, 4096, 1, G, nG, W, nW}, {"dWx    NT 576x4096x8000 ", 576, 4096, R, 4, X, nX, G, nG},
                         {"dWx    NT 1024x4096x8000", 1024, 4096, R, 2, X, nX, G, nG}, {"dU     NT 512x2048x8000 ", 512, 2048, R, 8, X, nX, G, nG},
                         {"odd    NT 1100x1024x4096", 1100, 1024, 4096, 1, G, nG, W, nW}};   // 192-row tiles, ragged last block row
  float* O2 = dev_rand((size_t)R * 4096);
  // ---- two fp16 planes + three products (gemm_tph.hip): the same shapes, operands scaled per row from measured maxima
  {
    CK(gemm_tph_prepare());
    unsigned char *HA, *HB;
    CK(hipMalloc(&HA, tph_bytes(R, 4096))); CK(hipMalloc(&HB, tph_bytes(4096, R)));
    float *sa, *ia, *sb, *ib, *sws;
    CK(hipMalloc(&sa, 8192 * 4)); CK(hipMalloc(&ia, 8192 * 4)); CK(hipMalloc(&sb, 8192 * 4)); CK(hipMalloc(&ib, 8192 * 4));
    CK(hipMalloc(&sws, tph_scale_ws_floats(8192, 8192) * 4));
    for (auto& c : nts) {
      if ((size_t)c.M * c.K > c.a_elems || (size_t)c.N * c.K > c.b_elems) continue;
      GemmDesc f{}; f.A = c.A; f.B = c.B; f.C = O2; f.M = c.M; f.N = c.N; f.K = c.K; f.lda = c.K; f.ldb = c.K; f.ldc = c.N;
      f.b_col = true; f.a_rows = c.M; f.split_k = 1;
      launch_gemm(f, st);
      float tsplit = 1e9f;
      for (int i = 0; i < 3; ++i) {
        CK(hipEventRecord(a, st));
        launch_tph_scales(c.A, c.M, c.K, c.K, sa, ia, nullptr, nullptr, sws, st);
        launch_tph_split2(c.A, HA, nullptr, c.M, c.K, c.K, sa, 1.f, nullptr, 1.f, nullptr, st);
        launch_tph_scales(c.B, c.N, c.K, c.K, sb, ib, nullptr, nullptr, sws, st);
        launch_tph_split2(c.B, HB, nullptr, c.N, c.K, c.K, sb, 1.f, nullptr, 1.f, nullptr, st);
        CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b)); tsplit = ms < tsplit ? ms : tsplit;
      }
      GemmTPHDesc g{}; g.A = HA; g.B = HB; g.C = O; g.M = c.M; g.N = c.N; g.K = c.K; g.nkbA = (c.K + 15) / 16; g.nkbB = g.nkbA; g.ldc = c.N;
      g.a_inv = ia; g.b_inv = ib;
      g.split_k = gemm_tph_pick_split(c.M, c.N, c.K); g.slabs = slabs;
      if ((size_t)g.split_k * c.M * c.N > (size_t)8 * 1024 * 4096) { printf("slabs too small\n"); continue; }
      CK(hipMemset(O, 0xff, (size_t)c.M * c.N * 4));
      launch_gemm_tph(g, st); CK(hipStreamSynchronize(st)); CK(hipGetLastError());
      std::vector<float> h1((size_t)c.M * c.N), h2((size_t)c.M * c.N);
      CK(hipMemcpy(h1.data(), O, h1.size() * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(h2.data(), O2, h2.size() * 4, hipMemcpyDeviceToHost));
      double num = 0, den = 0, mx = 0;
      for (size_t i = 0; i < h1.size(); ++i) { double d = (double)h1[i] - h2[i]; num += d * d; den += (double)h2[i] * h2[i]; if (!(fabs(d) <= mx)) mx = fabs(d); }
      float best = 1e9f;
      for (int i = 0; i < 10; ++i) {
        CK(hipEventRecord(a, st)); launch_gemm_tph(g, st); CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b));
        float ms; CK(hipEventElapsedTime(&ms, a, b)); best = ms < best ? ms : best;
      }
      printf("tph    %s split %d : %.3f ms  %.1f TF-equiv (+ %.3f ms for scales + planes of both operands)  rel-L2 vs f32 kernel %.2e  max abs %.2e\n", c.name, g.split_k, best,
             2.0 * c.M * c.N * c.K / best / 1e9, tsplit, sqrt(num / den), mx);
      if (getenv("NASR_SWEEP")) {
        for (int sp : {1, 2, 3, 4, 5, 6, 8, 10, 12, 16}) {
          if ((size_t)sp * c.M * c.N > (size_t)8 * 1024 * 4096 || (c.K + 15) / 16 / sp < 16) continue;
          g.split_k = sp;
          float b2 = 1e9f;
          launch_gemm_tph(g, st);
          for (int i = 0; i < 8; ++i) {
            CK(hipEventRecord(a, st)); launch_gemm_tph(g, st); CK(hipEventRecord(b, st)); CK(hipEventSynchronize(b));
            float ms; CK(hipEventElapsedTime(&ms, a, b)); b2 = ms < b2 ? ms : b2;
          }
          printf("   sweep %s split %2d : %.3f ms\n", c.name, sp, b2);
        }
      }
    }
  }
  {  // fp16-plane helpers against the host: scales (rows and columns of a ragged, wide-range matrix) and column sums
    const int rr = 960, kk = 1000, ld = 1024;
    std::vector<float> hx((size_t)rr * ld);
    CK(hipMemcpy(hx.data(), X, hx.size() * 4, hipMemcpyDeviceToHost));
    for (int r = 0; r < rr; ++r) for (int c = 0; c < kk; ++c) hx[(size_t)r * ld + c] *= ldexpf(1.f, (r * 7 + c * 3) % 40 - 20);
    for (int c = 0; c < kk; ++c) hx[(size_t)5 * ld + c] = 0.f;       // an all-zero row
    float* dx; CK(hipMalloc(&dx, hx.size() * 4)); CK(hipMemcpy(dx, hx.data(), hx.size() * 4, hipMemcpyHostToDevice));
    float *rs, *ri, *cs, *ci, *ws2, *cpart, *csum;
    CK(hipMalloc(&rs, rr * 4)); CK(hipMalloc(&ri, rr * 4)); CK(hipMalloc(&cs, kk * 4)); CK(hipMalloc(&ci, kk * 4));
    CK(hipMalloc(&ws2, tph_scale_ws_floats(rr, kk) * 4)); CK(hipMalloc(&cpart, (size_t)tp_split2_parts(rr) * kk * 4)); CK(hipMalloc(&csum, kk * 4));
    unsigned char *pn, *pt; CK(hipMalloc(&pn, tph_bytes(rr, kk))); CK(hipMalloc(&pt, tph_bytes(kk, rr)));
    launch_tph_scales(dx, rr, kk, ld, rs, ri, cs, ci, ws2, st);
    launch_tph_split2(dx, pn, pt, rr, kk, ld, rs, 1.f, cs, 1.f, cpart, st);
    launch_colsum_parts(cpart, tp_split2_parts(rr), kk, csum, st);
    CK(hipStreamSynchronize(st)); CK(hipGetLastError());
    std::vector<float> hrs(rr), hri(rr), hcs(kk), hci(kk), hsum(kk);
    CK(hipMemcpy(hrs.data(), rs, rr * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hri.data(), ri, rr * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hcs.data(), cs, kk * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(hci.data(), ci, kk * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hsum.data(), csum, kk * 4, hipMemcpyDeviceToHost));
    int badr = 0, badc = 0; double se = 0, sn = 0;
    for (int r = 0; r < rr; ++r) {
      float m = 0; for (int c = 0; c < kk; ++c) m = fmaxf(m, fabsf(hx[(size_t)r * ld + c]));
      const float v = m * hrs[r];
      if (!(m == 0 ? hrs[r] == 1.f : (v >= 16384.f && v < 32768.f)) || hrs[r] * hri[r] != 1.f) ++badr;
    }
    for (int c = 0; c < kk; ++c) {
      float m = 0; double sum = 0;
      for (int r = 0; r < rr; ++r) { m = fmaxf(m, fabsf(hx[(size_t)r * ld + c])); sum += hx[(size_t)r * ld + c]; }
      const float v = m * hcs[c];
      if (!(v >= 16384.f && v < 32768.f) || hcs[c] * hci[c] != 1.f) ++badc;
      se += (hsum[c] - sum) * (hsum[c] - sum); sn += sum * sum;
    }
    // planes back to values: element (r, c) of the normal planes
    std::vector<unsigned char> hp(tph_bytes(rr, kk)), hq(tph_bytes(kk, rr));
    CK(hipMemcpy(hp.data(), pn, hp.size(), hipMemcpyDeviceToHost)); CK(hipMemcpy(hq.data(), pt, hq.size(), hipMemcpyDeviceToHost));
    auto at = [&](const std::vector<unsigned char>& pl, int nkb, int row, int k) {
      const size_t tile = ((size_t)(row >> 5) * nkb + (k >> 4)) * 2 * 1024;
      const int r = row & 31, hh = (k >> 3) & 1, e = k & 7;
      const size_t off = tile + ((((r << 1) | (hh ^ ((r >> 3) & 1))) << 4)) + e * 2;
      _Float16 h1, h2; memcpy(&h1, &pl[off], 2); memcpy(&h2, &pl[off + 1024], 2);
      return (double)(float)h1 + (double)(float)h2;
    };
    // an element within 2^-18 of its line's maximum keeps 2^-23 relative; below that the error is 2^-39 of the maximum
    // (the printed ratio is against half of that bound: <= 2.00 expected)
    double worst_n = 0, worst_t = 0;
    for (int r = 0; r < rr; r += 7) for (int c = 0; c < kk; c += 3) {
      const double x = hx[(size_t)r * ld + c];
      if (x == 0) continue;
      const double bn = fmax(fabs(x) * ldexp(1.0, -24), ldexp(1.0, -40) * 32768.0 / hrs[r]);
      const double bt = fmax(fabs(x) * ldexp(1.0, -24), ldexp(1.0, -40) * 32768.0 / hcs[c]);
      worst_n = fmax(worst_n, fabs(at(hp, (kk + 15) / 16, r, c) / hrs[r] - x) / bn);
      worst_t = fmax(worst_t, fabs(at(hq, (rr + 15) / 16, c, r) / hcs[c] - x) / bt);
    }
    printf("fp16 planes of a 960x1000 matrix spanning 2^-20..2^20: %d / %d bad row / column scales, column sums rel %.1e, worst element error / bound max(2^-24 |x|, 2^-40 line max): %.2f (row-scaled planes) %.2f (column-scaled planes)\n",
           badr, badc, sqrt(se / sn), worst_n, worst_t);
  }
  return 0;
}
#endif
