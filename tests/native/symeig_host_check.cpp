// Host build of lvi-exc_amd/csrc/lvx_symeig.h (g++, one lane, no barrier): the Jacobi eigen-solver k_calib_cov runs in LDS, on matrices from a file.
//   symeig_host_check IN OUT
// IN : int32 count, then per matrix  int32 n, int32 max_sweeps, double A[n * n] (row-major, symmetric)
// OUT: per matrix  int32 rc, int32 sweeps, double off, double w[n] (ascending), double V[n * n] (row-major, column k = eigenvector of w[k])
// Stand-alone (its own main), so the same source can be built with -fsanitize=address,undefined and run as it is.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../lvi-exc_amd/csrc/lvx_symeig.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fi ? fopen(argv[2], "wb") : nullptr;
  if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
  int32_t count = 0;
  if (fread(&count, 4, 1, fi) != 1) return 3;
  for (int32_t m = 0; m < count; ++m) {
    int32_t hd[2];
    if (fread(hd, 4, 2, fi) != 2) return 3;
    const int n = hd[0];
    if (n < 1 || n > LVX_SYMEIG_MAX) { fprintf(stderr, "matrix %d: n = %d\n", (int)m, n); return 3; }
    std::vector<double> A((size_t)n * n), V((size_t)n * n), w(n), Vs((size_t)n * n);
    if (fread(A.data(), 8, A.size(), fi) != A.size()) return 3;
    double cs[LVX_SYMEIG_CS];
    int sweeps = 0; double off = 0.0;
    const int32_t rc = lvx::symeig_jacobi(A.data(), n, n, V.data(), n, cs, hd[1], 0, 1, lvx::SymeigNoSync(), &sweeps, &off);
    int order[LVX_SYMEIG_MAX];
    lvx::symeig_order(A.data(), n + 1, n, order);
    for (int k = 0; k < n; ++k) { w[k] = A[(size_t)order[k] * (n + 1)]; for (int i = 0; i < n; ++i) Vs[(size_t)i * n + k] = V[(size_t)i * n + order[k]]; }
    const int32_t head[2] = {rc, sweeps};
    fwrite(head, 4, 2, fo); fwrite(&off, 8, 1, fo); fwrite(w.data(), 8, w.size(), fo); fwrite(Vs.data(), 8, Vs.size(), fo);
  }
  fclose(fi);
  return fclose(fo) == 0 ? 0 : 4;
}
