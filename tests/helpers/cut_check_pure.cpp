// The check of sd_ahc_cut_grouped, alone: csrc/cut/sd_cut_check.h in a plain C++ program (no HIP header, no library), built with the
// address and undefined-behaviour sanitizers by tests/test_ahc_cut_rules.py.  Every argument is one call,
//     n_groups:n_merges:n_rows:cos_thr:ws_bytes:flags
// (cos_thr as strtof reads it, "nan" and "-inf" included; ws_bytes -1: what the call needs; flags: letters of t = a null table pointer,
// e = a null merge pointer, r = null labels, w = a null workspace, m = a misaligned workspace, or -), answered by one line:
// "status=0 need=BYTES" or "status=CODE why=TEXT".  "size:n_rows:n_groups" prints what sd_ahc_cut_workspace_bytes returns.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "cut/sd_cut_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int g = 0, e = 0, n = 0;
    long long ws = 0;
    char thr[32] = "", flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d", &n, &g) == 2) {
      printf("%zu\n", sd_cut_workspace_bytes(n, g));
      continue;
    }
    if (sscanf(argv[i], "%d:%d:%d:%31[^:]:%lld:%7s", &g, &e, &n, thr, &ws, flags) != 6) {
      fprintf(stderr, "bad call: %s\n", argv[i]);
      return 2;
    }
    SdCutCall c = {};
    c.n_groups = g, c.n_merges = e, c.n_rows = n;
    c.cos_thr = strtof(thr, nullptr);
    c.table_null = strchr(flags, 't') != nullptr;
    c.merges_null = strchr(flags, 'e') != nullptr;
    c.rows_null = strchr(flags, 'r') != nullptr;
    c.ws_null = strchr(flags, 'w') != nullptr;
    c.ws_misaligned = strchr(flags, 'm') != nullptr;
    char why[SD_CUT_WHY] = "";
    c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_cut_check(c, why, true) == SD_OK ? sd_cut_need(c) : 0);
    const int status = sd_cut_check(c, why);
    if (status != SD_OK) printf("status=%d why=%s\n", status, why);
    else printf("status=0 need=%zu\n", sd_cut_need(c));
  }
  return 0;
}
