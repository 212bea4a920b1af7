// stand-alone host check of the launch log: 8 threads note labels while the main thread toggles and reads
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>
#include "sd_hip_trace.h"
extern std::atomic<int> sd_launch_log_state;
void sd_launch_log_note(const char* label);
int main() {
  static const char* const labels[] = {"a_kernel", "b_kernel<1>", "c_kernel<x>/walk", "a_kernel"};
  if (sd_launch_log_enable(1) != 0) return 2;
  std::vector<std::thread> th;
  for (int t = 0; t < 8; ++t)
    th.emplace_back([t] { for (int i = 0; i < 20000; ++i) if (sd_launch_log_state.load(std::memory_order_relaxed)) sd_launch_log_note(labels[(i + t) % 4]); });
  char buf[256];
  for (int i = 0; i < 200; ++i) { (void)sd_launch_log_read(buf, sizeof buf); (void)sd_launch_log_read(buf, 5); }
  for (auto& x : th) x.join();
  size_t need = sd_launch_log_read(buf, sizeof buf);
  printf("%s(need %zu)\n", buf, need);
  long long a = 0, b = 0, c = 0;
  sscanf(buf, "a_kernel\t%lld\nb_kernel<1>\t%lld\nc_kernel<x>/walk\t%lld\n", &a, &b, &c);
  if (a + b + c != 160000 || a != 80000) { printf("FAIL counts\n"); return 1; }
  char small[4]; if (sd_launch_log_read(small, sizeof small) != need || small[3] != 0) { printf("FAIL short\n"); return 1; }
  if (sd_launch_log_enable(1) != 1 || sd_launch_log_read(buf, sizeof buf) != 1) { printf("FAIL clear\n"); return 1; }
  sd_launch_log_enable(0);
  printf("ok\n");
  return 0;
}
