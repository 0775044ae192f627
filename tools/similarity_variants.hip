// Throw-away comparison for profiles/column_similarity_notes.md: nvt_row_similarity (the library's
// W-lane search) against two kernels that exist ONLY here:
//   merge1   one lane per data row, serial two-pointer merge of the two CSR rows (what the
//            reference's numba kernel does) -- the design the library does not take
//   lds64    the W = 64 search with the longer row's column indices staged in LDS first
// Build:  hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include tools/similarity_variants.hip \
//             -L nvtabular_amd -lnvt_hip -Wl,-rpath,'$ORIGIN/../nvtabular_amd' -o tools/similarity_variants
// Run:    tools/similarity_variants short|long [reps]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nvt_hip.h"

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                  \
      exit(2);                                                                 \
    }                                                                          \
  } while (0)

__global__ __launch_bounds__(256) void merge1_kernel(const int32_t *a, const int32_t *b, uint64_t n, nvt_csr L,
                                                     nvt_csr R, double *out) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int64_t p = L.indptr[a[i]], pe = L.indptr[a[i] + 1], q = R.indptr[b[i]], qe = R.indptr[b[i] + 1];
  double acc = 0.0;
  while (p < pe && q < qe) {
    const int32_t x = L.indices[p], y = R.indices[q];
    if (x == y) acc += L.weights[p++] * R.weights[q++];
    else if (x < y) ++p;
    else ++q;
  }
  out[i] = acc;
}

constexpr int kStage = 2048;  // staged indices per group: 8 KiB, 32 KiB per workgroup
__global__ __launch_bounds__(256) void lds64_kernel(const int32_t *a, const int32_t *b, uint64_t n, nvt_csr L,
                                                    nvt_csr R, double *out) {
  __shared__ int32_t stage[4][kStage];
  const unsigned sub = threadIdx.x & 63, grp = threadIdx.x >> 6;
  for (uint64_t i = (uint64_t)blockIdx.x * 4 + grp; i < n; i += (uint64_t)gridDim.x * 4) {
    const int64_t pa = L.indptr[a[i]], la = L.indptr[a[i] + 1] - pa, pb = R.indptr[b[i]], lb = R.indptr[b[i] + 1] - pb;
    const bool ls = la <= lb;
    const int32_t *si = ls ? L.indices + pa : R.indices + pb, *li = ls ? R.indices + pb : L.indices + pa;
    const double *sw = ls ? L.weights + pa : R.weights + pb, *lw = ls ? R.weights + pb : L.weights + pa;
    const int64_t s = ls ? la : lb, l = ls ? lb : la;
    const bool staged = l <= kStage;
    if (staged)
      for (int64_t k = sub; k < l; k += 64) stage[grp][k] = li[k];
    __threadfence_block();  // (one wave fills and reads its slice: no barrier)
    const int32_t *look = staged ? stage[grp] : li;
    double acc = 0.0;
    for (int64_t k = sub; k < s; k += 64) {
      const int32_t c = si[k];
      int64_t lo = 0, len = l;
      while (len > 0) {
        const int64_t half = len >> 1;
        if (look[lo + half] < c) lo += half + 1, len -= half + 1;
        else len = half;
      }
      if (lo < l && look[lo] == c) acc += sw[k] * lw[lo];
    }
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (sub == 0) out[i] = acc;
  }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33);
}

int main(int argc, char **argv) {
  const bool is_long = argc > 1 && !strcmp(argv[1], "long");
  const int reps = argc > 2 ? atoi(argv[2]) : 5;
  const uint64_t rows = is_long ? 100000 : 3000000, cols = is_long ? 10000 : 100, n = is_long ? 5000000 : 40000000;
  std::vector<int64_t> indptr(rows + 1, 0);
  std::vector<int32_t> indices;
  std::vector<double> weights;
  for (uint64_t r = 0; r < rows; ++r) {
    if (is_long) {
      int32_t c = -1;
      for (int k = 0; k < 200; ++k) indices.push_back(c += 1 + rnd() % 49);
    } else {
      int32_t pick[5];
      const int k = 1 + rnd() % 5;
      for (int j = 0; j < k;) {
        pick[j] = rnd() % cols;
        if (std::find(pick, pick + j, pick[j]) == pick + j) ++j;
      }
      std::sort(pick, pick + k);
      indices.insert(indices.end(), pick, pick + k);
    }
    indptr[r + 1] = (int64_t)indices.size();
  }
  for (size_t k = 0; k < indices.size(); ++k) weights.push_back(0.25 + (rnd() % 1024) / 512.0);
  std::vector<int32_t> a(n), b(n);
  for (uint64_t i = 0; i < n; ++i) a[i] = rnd() % rows, b[i] = rnd() % rows;
  const uint64_t nnz = indices.size();

  int64_t *d_ptr;
  int32_t *d_idx, *d_a, *d_b;
  double *d_w, *d_out[3];
  void *ws;
  uint64_t ws_bytes = 0;
  if (nvt_row_similarity_ws_bytes(n, &ws_bytes)) return 2;
  CK(hipMalloc(&d_ptr, (rows + 1) * 8));
  CK(hipMalloc(&d_idx, nnz * 4));
  CK(hipMalloc(&d_w, nnz * 8));
  CK(hipMalloc(&d_a, n * 4));
  CK(hipMalloc(&d_b, n * 4));
  CK(hipMalloc(&ws, ws_bytes));
  for (auto &o : d_out) CK(hipMalloc(&o, n * 8));
  CK(hipMemcpy(d_ptr, indptr.data(), (rows + 1) * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_idx, indices.data(), nnz * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_w, weights.data(), nnz * 8, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_a, a.data(), n * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_b, b.data(), n * 4, hipMemcpyHostToDevice));
  const nvt_csr m{d_ptr, d_idx, d_w, rows};
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const char *names[3] = {"library", "merge1", "lds64"};
  const int nvar = is_long ? 3 : 2;  // (lds64 serves W = 64 rows only: the long case)
  printf("case %s: matrix %llu x %llu, nnz %llu, %llu data rows\n", is_long ? "long" : "short",
         (unsigned long long)rows, (unsigned long long)cols, (unsigned long long)nnz, (unsigned long long)n);
  for (int rep = -1; rep < reps; ++rep) {  // rep -1 warms every variant up; then they alternate
    for (int v = 0; v < nvar; ++v) {
      CK(hipEventRecord(e0, nullptr));
      if (v == 0) {
        if (nvt_row_similarity(d_a, nullptr, d_b, nullptr, NVT_I32, n, &m, &m, d_out[0], ws, ws_bytes, nullptr)) {
          fprintf(stderr, "%s\n", nvt_last_error());
          return 2;
        }
      } else if (v == 1) {
        merge1_kernel<<<(unsigned)((n + 255) / 256), 256>>>(d_a, d_b, n, m, m, d_out[1]);
      } else {
        lds64_kernel<<<2048, 256>>>(d_a, d_b, n, m, m, d_out[2]);
      }
      CK(hipEventRecord(e1, nullptr));
      CK(hipEventSynchronize(e1));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      if (rep >= 0) printf("rep %d %-8s %9.3f ms  %8.1f M rows/s\n", rep, names[v], ms, n / ms / 1e3);
    }
  }
  std::vector<double> ref(n), got(n);
  CK(hipMemcpy(ref.data(), d_out[1], n * 8, hipMemcpyDeviceToHost));
  for (int v : {0, 2}) {
    if (v >= nvar) continue;
    CK(hipMemcpy(got.data(), d_out[v], n * 8, hipMemcpyDeviceToHost));
    double worst = 0;
    for (uint64_t i = 0; i < n; ++i) worst = std::max(worst, std::abs(got[i] - ref[i]));
    printf("max |%s - merge1| = %.3g\n", names[v], worst);
  }
  return 0;
}
