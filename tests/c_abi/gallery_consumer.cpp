// 1:N identification through the C ABI alone (include/efm_hip.h + the HIP runtime for memory): pack a 100-row gallery, scan it as two
// chunks of 50 rows into one workspace, merge, and check answers known by construction — in fp32 and bf16 storage, row and identity
// mode.  Build:  hipcc -std=c++17 -I include tests/c_abi/gallery_consumer.cpp -L <pkg dir> -lefm_hip -o gallery_consumer
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <vector>

#include "efm_hip.h"

#define CK(x)                                                                 \
  do {                                                                        \
    hipError_t e_ = (x);                                                      \
    if (e_ != hipSuccess) { std::printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } \
  } while (0)
#define EFM(x)                                                                \
  do {                                                                        \
    int rc_ = (x);                                                            \
    if (rc_ != EFM_OK) { std::printf("efm error %d: %s at %s:%d\n", rc_, efm_last_error_string(), __FILE__, __LINE__); return 3; } \
  } while (0)
#define EXPECT(c)                                                             \
  do {                                                                        \
    if (!(c)) { std::printf("check failed: %s (line %d)\n", #c, __LINE__); return 4; } \
  } while (0)

int main() {
  const int N = 100, D = 20, LD = 32, NQ = 3, K = 3, CHUNK = 50;
  // row i points along axis i % 20 with length 1 + i / 20 (any norm: pack normalises); identity of row i = i / 10
  std::vector<float> g((size_t)N * D, 0.f), q((size_t)NQ * D, 0.f);
  std::vector<int32_t> labels(N);
  for (int i = 0; i < N; ++i) {
    g[(size_t)i * D + i % D] = 1.f + i / D;
    labels[i] = i / 10;
  }
  q[0 * D + 3] = 1.f;    // query 0: axis 3 -> rows 3, 23, 43, 63, 83 all score 1; ties go to the lower row
  q[1 * D + 17] = 4.f;   // query 1: axis 17 -> rows 17, 37, 57 ...
  // query 2: zero -> matches nothing
  float *dg, *dq;
  int32_t* dl;
  void* packed;
  CK(hipMalloc(&dg, g.size() * 4));
  CK(hipMalloc(&dq, q.size() * 4));
  CK(hipMalloc(&dl, N * 4));
  CK(hipMalloc(&packed, (size_t)N * LD * 4));
  CK(hipMemcpy(dg, g.data(), g.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dl, labels.data(), N * 4, hipMemcpyHostToDevice));
  const size_t ws_bytes = efm_gallery_workspace_bytes(NQ, 2, K);
  EXPECT(ws_bytes > 0 && efm_gallery_workspace_bytes(NQ, 2, 33) == 0);
  void* ws;
  CK(hipMalloc(&ws, ws_bytes));
  float* ds;
  int32_t *di, *dlab;
  CK(hipMalloc(&ds, NQ * K * 4));
  CK(hipMalloc(&di, NQ * K * 4));
  CK(hipMalloc(&dlab, NQ * K * 4));
  for (int bf16 = 0; bf16 <= 1; ++bf16) {
    const size_t es = bf16 ? 2 : 4;
    EFM(efm_gallery_pack(dg, N, D, D, packed, bf16, LD, nullptr));
    for (int by_label = 0; by_label <= 1; ++by_label) {
      for (int c = 0; c < 2; ++c)
        EFM(efm_gallery_scan(dq, NQ, D, D, (const char*)packed + (size_t)c * CHUNK * LD * es, bf16, CHUNK, LD,
                             by_label ? dl + c * CHUNK : nullptr, (int64_t)c * CHUNK, K, 0.5f, ws, c, nullptr));
      EFM(efm_gallery_merge(ws, 2, NQ, K, by_label, ds, di, dlab, nullptr));
      std::vector<float> s(NQ * K);
      std::vector<int32_t> idx(NQ * K), lab(NQ * K);
      CK(hipMemcpy(s.data(), ds, s.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(idx.data(), di, idx.size() * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(lab.data(), dlab, lab.size() * 4, hipMemcpyDeviceToHost));
      // row mode: the three lowest rows on the axis; identity mode: rows 3 / 23 / 43 are identities 0 / 2 / 4 (one row each here)
      const int want0[K] = {3, 23, 43}, want1[K] = {17, 37, 57};
      for (int j = 0; j < K; ++j) {
        EXPECT(idx[0 * K + j] == want0[j] && std::fabs(s[0 * K + j] - 1.f) < 1e-6f);
        EXPECT(idx[1 * K + j] == want1[j] && std::fabs(s[1 * K + j] - 1.f) < 1e-6f);
        EXPECT(idx[2 * K + j] == -1 && std::isinf(s[2 * K + j]) && s[2 * K + j] < 0 && lab[2 * K + j] == -1);
        if (by_label) {
          EXPECT(lab[0 * K + j] == want0[j] / 10 && lab[1 * K + j] == want1[j] / 10);
        } else {
          EXPECT(lab[0 * K + j] == -1);
        }
      }
    }
  }
  // an argument outside the limits is refused with a message, not launched
  EXPECT(efm_gallery_scan(dq, NQ, D, D, packed, 0, N, 20, nullptr, 0, K, 0.f, ws, 0, nullptr) == EFM_E_INVALID);
  CK(hipFree(dg));
  CK(hipFree(dq));
  CK(hipFree(dl));
  CK(hipFree(packed));
  CK(hipFree(ws));
  CK(hipFree(ds));
  CK(hipFree(di));
  CK(hipFree(dlab));
  std::printf("gallery consumer: OK\n");
  return 0;
}
