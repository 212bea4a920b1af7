// The check of sd_kmeans_grouped_f64, alone: csrc/kmeans/sd_kmeans_check.h in a plain C++ program (no HIP header, no library), built
// with the address and undefined-behaviour sanitizers by tests/test_kmeans_rules.py.  Every argument is one call,
//     n_rows:dim:ld:n_groups:n_init:max_iter:max_k:max_rows:tol_rel:ws_bytes:flags
// (tol_rel as strtod reads it, "nan" and "inf" included; ws_bytes -1: what the call needs; flags: letters of t = a null table pointer,
// r = null rows or labels, a = misaligned rows, m = a misaligned workspace, or -), answered by one line: "status=0 need=BYTES" or
// "status=CODE why=TEXT".  "size:n_rows:n_groups:n_init" prints what sd_kmeans_grouped_workspace_bytes returns, "lds:dim:max_k:max_rows"
// the doubles of LDS before the rows and those the rows may take.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kmeans/sd_kmeans_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int n = 0, d = 0, g = 0, r = 0, it = 0, mk = 0, mr = 0;
    long ld = 0;
    long long ws = 0;
    char tol[32] = "", flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d:%d", &n, &g, &r) == 3) {
      printf("%zu\n", sd_kmeans_workspace_bytes(n, g, r));
      continue;
    }
    if (sscanf(argv[i], "lds:%d:%d:%d", &d, &mk, &mr) == 3) {
      printf("%d %d\n", sd_km_fixed_doubles(d, mk), sd_km_rows_cap(d, mk, mr));
      continue;
    }
    if (sscanf(argv[i], "%d:%d:%ld:%d:%d:%d:%d:%d:%31[^:]:%lld:%7s", &n, &d, &ld, &g, &r, &it, &mk, &mr, tol, &ws, flags) != 11) {
      fprintf(stderr, "bad call: %s\n", argv[i]);
      return 2;
    }
    SdKmeansCall c = {};
    c.n_rows = n, c.dim = d, c.ld = ld, c.n_groups = g, c.n_init = r, c.max_iter = it, c.max_k = mk, c.max_rows = mr;
    c.tol_rel = strtod(tol, nullptr);
    c.table_null = strchr(flags, 't') != nullptr;
    c.rows_null = strchr(flags, 'r') != nullptr;
    c.rows_misaligned = strchr(flags, 'a') != nullptr;
    c.ws_misaligned = strchr(flags, 'm') != nullptr;
    char why[SD_KMEANS_WHY] = "";
    c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_kmeans_check(c, why, true) == SD_OK ? sd_kmeans_need(c) : 0);
    const int status = sd_kmeans_check(c, why);
    if (status != SD_OK) printf("status=%d why=%s\n", status, why);
    else printf("status=0 need=%zu\n", sd_kmeans_need(c));
  }
  return 0;
}
