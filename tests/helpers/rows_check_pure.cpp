// The check of the entries that take f32 rows, alone: csrc/sd_rows_check.h in a plain C++ program (no HIP header, no library), built
// with the address and undefined-behaviour sanitizers by tests/test_rows_check_rules.py.  Every argument is one call,
//     entry:n:d:ld:k:ld2:ld3:ws_bytes:flags
// (entry: nearest merge grouped core outgoing stats apply centroids, described as the entry of that name describes itself; k: k or
// max_group; ld2, ld3: ldg | ldw, ldo | ldo; ld, ld2, ld3 -1: d rounded up to four; ws_bytes -1: what the call needs; flags: letters of
// p = a null pointer, r = misaligned rows, m = misaligned workspace, or -), answered by one line: "status=0 need=BYTES" or
// "status=CODE why=TEXT".  "size:entry:n:d:k" prints what the entry's *_workspace_bytes function returns.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sd_rows_check.h"

static bool describe(const char* entry, int n, int d, long ld, int k, long ld2, long ld3, SdRowsCall* c) {
  if (!strcmp(entry, "nearest")) *c = {"sd_ahc_nearest_f32", "sums", SD_ROWS_SYM, n, d, ld, 1, GT_MAX_D};
  else if (!strcmp(entry, "merge")) *c = {"sd_ahc_merge_f32", "sums", SD_ROWS_ONLY, n, d, ld, 1, INT_MAX};
  else if (!strcmp(entry, "grouped")) *c = {"sd_ahc_nearest_grouped_f32", "sums", SD_ROWS_BAND, n, d, ld, 1, GT_MAX_D, k};
  else if (!strcmp(entry, "core")) *c = {"sd_hdb_core_f32", "rows", SD_ROWS_CORE, n, d, ld, 1, GT_MAX_D, k};
  else if (!strcmp(entry, "outgoing")) *c = {"sd_hdb_outgoing_f32", "rows", SD_ROWS_SYM, n, d, ld, 1, GT_MAX_D};
  else if (!strcmp(entry, "stats")) *c = {"sd_whiten_stats_f64", "x", SD_ROWS_WHITEN, n, d, ld, 2, DG_MAX_D, 0, {{"ldg", ld2}}};
  else if (!strcmp(entry, "apply")) *c = {"sd_whiten_apply_f64", "x", SD_ROWS_ONLY, n, d, ld, 1, DG_MAX_D, 0, {{"ldw", ld2}, {"ldo", ld3}}};
  else if (!strcmp(entry, "centroids")) *c = {"sd_label_centroids_f32", "x", SD_ROWS_LABELS, n, d, ld, 1, DG_MAX_D, k, {{"ldo", ld2}}};
  else return false;
  return true;
}

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    char entry[16] = "", flags[8] = "";
    int n = 0, d = 0, k = 0;
    long ld = 0, ld2 = 0, ld3 = 0;
    long long ws = 0;
    SdRowsCall c = {};
    if (sscanf(argv[i], "size:%15[^:]:%d:%d:%d", entry, &n, &d, &k) == 4) {
      if (!describe(entry, n, d, 0, k, 0, 0, &c)) return 2;
      printf("%zu\n", sd_rows_workspace_bytes(c.kind, n, d, c.min_n, c.max_d, k));
      continue;
    }
    if (sscanf(argv[i], "%15[^:]:%d:%d:%ld:%d:%ld:%ld:%lld:%7s", entry, &n, &d, &ld, &k, &ld2, &ld3, &ws, flags) != 9) {
      fprintf(stderr, "bad call: %s\n", argv[i]);
      return 2;
    }
    const long wide = ((long)d + 3) / 4 * 4;
    if (!describe(entry, n, d, ld == -1 ? wide : ld, k, ld2 == -1 ? wide : ld2, ld3 == -1 ? wide : ld3, &c)) {
      fprintf(stderr, "bad entry: %s\n", argv[i]);
      return 2;
    }
    c.any_null = strchr(flags, 'p') != nullptr;
    c.rows_misaligned = strchr(flags, 'r') != nullptr;
    c.ws_misaligned = strchr(flags, 'm') != nullptr;
    char why[SD_ROWS_WHY] = "";
    if (ws >= 0) c.ws_bytes = (size_t)ws;
    else c.ws_bytes = sd_rows_check(c, why, true) == SD_OK ? sd_rows_need(c) : 0;      // what the call needs, where its shape has a need at all
    const int status = sd_rows_check(c, why);
    if (status != SD_OK) printf("status=%d why=%s\n", status, why);
    else printf("status=0 need=%zu\n", sd_rows_need(c));
  }
  return 0;
}
