// The check of sd_scd_split_grouped_f32, alone: csrc/scd/sd_scd_check.h in a plain C++ program (no HIP header, no library), built
// with the address and undefined-behaviour sanitizers by tests/test_scd_rules.py.  Every argument is one call:
//     split:ld:dim:n_rows:n_segs:piece_cap:hop_ms:thr:min_speech_s:eps:ws_bytes:flags
//                                              ws_bytes -1: what the call needs; flags: letters of t = a null table pointer,
//                                              r = null rows or ws, p = null piece_start or piece_end, m = a misaligned workspace, or -
// (floats as strtod reads them, "nan" and "inf" included), answered by one line: "status=0 need=BYTES" or "status=CODE why=TEXT".
// "size:n_rows:n_segs" prints what sd_scd_split_workspace_bytes returns, "layout" the constants of the kernel, "cap:n" the piece
// capacity of a segment of n rows, "offsets:n_rows" the byte offsets of the distances and of the chain in the workspace.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scd/sd_scd_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int ld = 0, dim = 0, rows = 0, segs = 0, cap = 0, n = 0;
    long long ws = 0;
    char a[32] = "", b[32] = "", c3[32] = "", d[32] = "", flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d", &rows, &segs) == 2) {
      printf("%zu\n", sd_scd_workspace_bytes(rows, segs));
      continue;
    }
    if (sscanf(argv[i], "cap:%d", &n) == 1) {
      printf("%d\n", sd_scd_piece_capacity(n));
      continue;
    }
    if (sscanf(argv[i], "offsets:%d", &rows) == 1) {
      printf("%zu %zu\n", sd_scd_ws_dist_offset(rows), sd_scd_ws_chain_offset(rows));
      continue;
    }
    if (strcmp(argv[i], "layout") == 0) {
      printf("%d %d %d\n", SD_SCD_THREADS, SD_SCD_S_LDS_ROWS, SD_SCD_S_LDS_CUTS);
      continue;
    }
    char why[SD_SCD_WHY] = "";
    if (sscanf(argv[i], "split:%d:%d:%d:%d:%d:%31[^:]:%31[^:]:%31[^:]:%31[^:]:%lld:%7s", &ld, &dim, &rows, &segs, &cap, a, b, c3, d, &ws, flags) == 11) {
      SdScdCall c = {};
      c.ld = ld, c.dim = dim, c.n_rows = rows, c.n_segs = segs, c.piece_cap = cap;
      c.hop_ms = strtod(a, nullptr), c.thr = strtod(b, nullptr), c.min_speech_s = strtod(c3, nullptr), c.eps = strtof(d, nullptr);
      c.table_null = strchr(flags, 't') != nullptr;
      c.rows_null = strchr(flags, 'r') != nullptr;
      c.pieces_null = strchr(flags, 'p') != nullptr;
      c.ws_misaligned = strchr(flags, 'm') != nullptr;
      c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_scd_check(c, why, true) == SD_OK ? sd_scd_need(c) : 0);
      const int status = sd_scd_check(c, why);
      if (status != SD_OK) printf("status=%d why=%s\n", status, why);
      else printf("status=0 need=%zu\n", sd_scd_need(c));
      continue;
    }
    fprintf(stderr, "bad call: %s\n", argv[i]);
    return 2;
  }
  return 0;
}
