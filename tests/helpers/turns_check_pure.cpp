// The check of sd_turns_grouped, alone: csrc/turns/sd_turns_check.h in a plain C++ program (no HIP header, no library), built with
// the address and undefined-behaviour sanitizers by tests/test_turns_rules.py.  Every argument is one call:
//     turns:n_recordings:n_regions:n_windows:frame_s:ws_bytes:flags
//                                              ws_bytes -1: what the call needs; flags: letters of t = a null table pointer, r = null
//                                              region_start or n_frames, w = a null [n_windows] array, n = a null workspace,
//                                              m = a misaligned workspace, or -
// (frame_s as strtod reads it, "nan" and "inf" included), answered by one line: "status=0 need=BYTES" or "status=CODE why=TEXT".
// "size:n_windows:n_recordings" prints what sd_turns_workspace_bytes returns, "layout" the constants of the kernel,
// "offset:n_windows" the byte offset of table B in the workspace.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "turns/sd_turns_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int recs = 0, regions = 0, windows = 0;
    long long ws = 0;
    char a[32] = "", flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d", &windows, &recs) == 2) {
      printf("%zu\n", sd_turns_ws_bytes(windows, recs));
      continue;
    }
    if (sscanf(argv[i], "offset:%d", &windows) == 1) {
      printf("%zu\n", sd_turns_ws_b_offset(windows));
      continue;
    }
    if (strcmp(argv[i], "layout") == 0) {
      printf("%d %d\n", SD_TURNS_THREADS, SD_TURNS_T_LDS_WINDOWS);
      continue;
    }
    char why[SD_TURNS_WHY] = "";
    if (sscanf(argv[i], "turns:%d:%d:%d:%31[^:]:%lld:%7s", &recs, &regions, &windows, a, &ws, flags) == 6) {
      SdTurnsCall c = {};
      c.n_recordings = recs, c.n_regions = regions, c.n_windows = windows, c.frame_s = strtod(a, nullptr);
      c.table_null = strchr(flags, 't') != nullptr;
      c.region_null = strchr(flags, 'r') != nullptr;
      c.window_null = strchr(flags, 'w') != nullptr;
      c.ws_null = strchr(flags, 'n') != nullptr;
      c.ws_misaligned = strchr(flags, 'm') != nullptr;
      c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_turns_check(c, why, true) == SD_OK ? sd_turns_need(c) : 0);
      const int status = sd_turns_check(c, why);
      if (status != SD_OK) printf("status=%d why=%s\n", status, why);
      else printf("status=0 need=%zu\n", sd_turns_need(c));
      continue;
    }
    fprintf(stderr, "bad call: %s\n", argv[i]);
    return 2;
  }
  return 0;
}
