// k_scan_cells on its own: random cell counts, some of them big buckets, many blocks; checks the bucket starts against a
// host prefix sum and the task list against the buckets -- also when the buckets have more tasks than the list holds
// (kMaxSortTasks): then every entry is a task of a bucket listed whole, or a no-op (cell -1) of the one bucket the list's
// end cuts, and no bucket is listed in part.  Counts only: no particles.
// hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -std=c++17
//   -Iinclude -Isand_crate_amd/csrc scripts/scan_check.hip -o scratch/scan_check
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <map>
#include "sc_device.h"
#include "sc_kernels.h"
using namespace sc;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int tasks_of(int e) { return (e + kSortChunk - 1) / kSortChunk; }
static int chunk_len(int e, int j) { return std::min(kSortChunk, e - j * kSortChunk); }

// `want_noop`, `want_out`: the no-op entries and the buckets left out that the counts imply, or -1: whatever the order of
// the atomics makes them (the other checks hold either way)
static int run_case(const std::vector<int>& cnt, int n, int want_noop, int want_out) {
  const int nb = (n + 1 + kScanPerBlock - 1) / kScanPerBlock;
  int *in, *out, *counters; unsigned long long* desc; int2* tasks;
  CK(hipMalloc((void**)&in, (n + 1) * 4)); CK(hipMalloc((void**)&out, (n + 2) * 4)); CK(hipMalloc((void**)&counters, C_ALLOC * 4));
  CK(hipMalloc((void**)&desc, (nb + 4) * 8)); CK(hipMalloc((void**)&tasks, kMaxSortTasks * 8));
  CK(hipMemset(desc, 0, (nb + 4) * 8));
  CK(hipMemcpy(in, cnt.data(), (n + 1) * 4, hipMemcpyHostToDevice));
  for (unsigned stamp = 1; stamp <= 3; ++stamp) {
    CK(hipMemset(counters, 0, C_ALLOC * 4));
    CK(hipMemset(tasks, 0xFF, kMaxSortTasks * 8));  // an entry nobody wrote: cell -1 and word -1, which no task packs
    hipLaunchKernelGGL(k_scan_cells, dim3(nb), dim3(kBlock), 0, 0, in, out, n, desc, stamp, counters, tasks, kScanMaxPolls);
    CK(hipDeviceSynchronize());
  }
  std::vector<int> got(n + 1), ctr(C_ALLOC); std::vector<int2> tk(kMaxSortTasks);
  CK(hipMemcpy(got.data(), out, (n + 1) * 4, hipMemcpyDeviceToHost)); CK(hipMemcpy(ctr.data(), counters, C_ALLOC * 4, hipMemcpyDeviceToHost));
  CK(hipMemcpy(tk.data(), tasks, kMaxSortTasks * 8, hipMemcpyDeviceToHost));
  long long run = 0; int bad = 0, nbig = 0, ntasks = 0;
  std::map<long long, int> want;  // (cell, chunk) -> length
  for (int i = 0; i <= n; ++i) {
    if (got[i] != run && bad++ < 3) printf("  start[%d] = %d, expected %lld\n", i, got[i], run);
    if (i < n) {
      run += cnt[i];
      if (cnt[i] > kSortThreshold) { ++nbig; for (int j = 0; j * kSortChunk < cnt[i]; ++j) { want[(long long)i << 20 | j] = chunk_len(cnt[i], j); ++ntasks; } }
    }
  }
  int tbad = 0;
  if (ctr[C_NBIG] != nbig || ctr[C_NTASKS] != ntasks || ctr[C_NT] != run) { printf("  counters: big %d (%d) tasks %d (%d) total %d (%lld) flags %d\n", ctr[C_NBIG], nbig, ctr[C_NTASKS], ntasks, ctr[C_NT], run, ctr[C_FLAGS]); ++tbad; }
  const int held = std::min(ntasks, kMaxSortTasks);
  std::map<int, int> listed;  // cell -> its tasks in the list
  std::vector<int2> noop;
  for (int t = 0; t < held; ++t) {
    const int chunk = tk[t].y & 0xFFFFF, len = (tk[t].y >> 20) + 1;
    if (tk[t].x == -1) {
      if (tk[t].y == -1) { if (tbad++ < 3) printf("  entry %d was never written\n", t); }
      else noop.push_back(make_int2(chunk, len));
      continue;
    }
    auto it = want.find((long long)tk[t].x << 20 | chunk);
    if (it == want.end() || it->second != len) { if (tbad++ < 3) printf("  task %d: cell %d chunk %d len %d unexpected\n", t, tk[t].x, chunk, len); }
    else { want.erase(it); ++listed[tk[t].x]; }
  }
  int whole_tasks = 0, out_buckets = nbig - (int)listed.size();
  for (const auto& [cell, k] : listed) {
    whole_tasks += k;
    if (k != tasks_of(cnt[cell])) { if (tbad++ < 3) printf("  cell %d is listed in part: %d of %d tasks\n", cell, k, tasks_of(cnt[cell])); }
  }
  if (ntasks <= kMaxSortTasks) {
    if (!want.empty()) { printf("  %zu tasks missing\n", want.size()); ++tbad; }
    if (!noop.empty()) { printf("  %zu no-op entries in a list with room for all\n", noop.size()); ++tbad; }
  } else {
    // the list is full: what is not a task of a whole bucket is a no-op, and those are the first chunks of ONE bucket that is
    // left out (ranges are handed out back to back: only one bucket can lie across the list's end)
    if (whole_tasks + (int)noop.size() != kMaxSortTasks) { printf("  %d tasks of whole buckets + %zu no-ops != %d\n", whole_tasks, noop.size(), kMaxSortTasks); ++tbad; }
    if ((long long)want.size() != ntasks - whole_tasks) { printf("  %zu tasks left out, expected %d\n", want.size(), ntasks - whole_tasks); ++tbad; }
    if (out_buckets < 1) { printf("  no bucket is left out of a list too short\n"); ++tbad; }
    bool found = noop.empty();
    for (int i = 0; i < n && !found; ++i) {
      if (cnt[i] <= kSortThreshold || listed.count(i) || tasks_of(cnt[i]) <= (int)noop.size()) continue;
      std::vector<int> seen(noop.size(), 0);
      bool ok = true;
      for (const int2& e : noop) ok = ok && e.x < (int)noop.size() && !seen[e.x]++ && e.y == chunk_len(cnt[i], e.x);
      found = ok;
    }
    if (!found) { printf("  the %zu no-ops are not the first chunks of a bucket that is left out\n", noop.size()); ++tbad; }
    if ((want_noop >= 0 && (int)noop.size() != want_noop) || (want_out >= 0 && out_buckets != want_out)) {
      printf("  %zu no-ops (%d), %d buckets left out (%d)\n", noop.size(), want_noop, out_buckets, want_out); ++tbad;
    }
  }
  printf("%8d cells, %5d big buckets, %d blocks: starts %s, tasks %s (%d)\n", n, nbig, nb, bad ? "WRONG" : "ok", tbad ? "WRONG" : "ok", ntasks);
  hipFree(in); hipFree(out); hipFree(counters); hipFree(desc); hipFree(tasks);
  return 0;
}

int main() {
  for (int n : {1000, 300000, 1200000, 5000000}) {
    for (int bigs : {0, 5, 3000}) {
      std::vector<int> cnt(n + 1, 0);
      srand(n + bigs);
      for (int i = 0; i < n; ++i) cnt[i] = rand() % 9;
      for (int b = 0; b < bigs; ++b) cnt[rand() % n] = 97 + rand() % 4000;
      if (run_case(cnt, n, -1, -1)) return 1;
    }
  }
  // lists that are full: 5,462 buckets of three tasks (16,386: one bucket is cut, one of its tasks inside the list), 16,384
  // buckets of one task (nothing is cut), 16,385 (one is left out, none of it inside the list)
  struct Full { int buckets, size, noop, out; };
  for (const Full f : {Full{5462, 2049, 1, 1}, Full{16384, 0, 0, 0}, Full{16385, 0, 0, 1}}) {
    const int n = 300000;
    std::vector<int> cnt(n + 1, 0), cells(n);
    srand(f.buckets);
    for (int i = 0; i < n; ++i) { cnt[i] = rand() % 9; cells[i] = i; }
    for (int b = 0; b < f.buckets; ++b) {  // distinct cells
      std::swap(cells[b], cells[b + rand() % (n - b)]);
      cnt[cells[b]] = f.size ? f.size : kSortThreshold + 1 + rand() % (kSortChunk - kSortThreshold);
    }
    if (run_case(cnt, n, f.noop, f.out)) return 1;
  }
  return 0;
}
