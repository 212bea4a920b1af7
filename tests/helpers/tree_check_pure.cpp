// The check of sd_tree_labels_grouped, alone: csrc/tree/sd_tree_check.h in a plain C++ program (no HIP header, no library), built with
// the address and undefined-behaviour sanitizers by tests/test_hdbscan_labels_rules.py.  Every argument is one call,
//     n_edges:n_groups:max_edges:min_cluster_size:allow_single_cluster:ws_bytes:flags
// (ws_bytes -1: what the call needs; flags: letters of p = a null pointer, w = a null workspace, d = misaligned dist, m = misaligned
// workspace, or -), answered by one line: "status=0 need=BYTES lds_rows=ROWS" or "status=CODE why=TEXT".  "size:n_edges:n_groups:max_edges"
// prints what sd_tree_labels_workspace_bytes returns.
#ifdef __HIP__
#error "the check must compile without HIP"
#endif
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tree/sd_tree_check.h"

int main(int argc, char** argv) {
  for (int i = 1; i < argc; ++i) {
    int e = 0, g = 0, m = 0, mcs = 0, single = 0;
    long long ws = 0;
    char flags[8] = "";
    if (sscanf(argv[i], "size:%d:%d:%d", &e, &g, &m) == 3) {
      printf("%zu\n", sd_tree_workspace_bytes(e, g, m));
      continue;
    }
    if (sscanf(argv[i], "%d:%d:%d:%d:%d:%lld:%7s", &e, &g, &m, &mcs, &single, &ws, flags) != 7) {
      fprintf(stderr, "bad call: %s\n", argv[i]);
      return 2;
    }
    SdTreeCall c = {e, g, m, mcs, single};
    c.any_null = strchr(flags, 'p') != nullptr;
    c.ws_null = strchr(flags, 'w') != nullptr;
    c.dist_misaligned = strchr(flags, 'd') != nullptr;
    c.ws_misaligned = strchr(flags, 'm') != nullptr;
    char why[SD_TREE_WHY] = "";
    c.ws_bytes = ws >= 0 ? (size_t)ws : (sd_tree_check(c, why, true) == SD_OK ? sd_tree_need(c) : 0);
    const int status = sd_tree_check(c, why);
    if (status != SD_OK) printf("status=%d why=%s\n", status, why);
    else printf("status=0 need=%zu lds_rows=%d\n", sd_tree_need(c), sd_tree_lds_rows(c.max_edges));
  }
  return 0;
}
