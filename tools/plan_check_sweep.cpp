// plan_check_sweep.cpp -- the checker of plan tables (csrc/plan_check.cpp) under the sanitizers, on the CPU.
//
//   make -C mpc-interface_amd plan-check-sweep
//   python tools/dump_plan_tables.py DIR && for p in DIR/*.itab; do tools/plan_check_sweep $p ${p%.itab}.dtab; done
//
// Reads the itab (int32) and dtab (float64) of a valid plan, as tools/dump_plan_tables.py writes them, into
// malloc'd blocks of their exact size, asserts that validate_plan accepts them, then sets every word of itab in
// turn to a handful of values -- the neighbours of the old one, small and large constants, the table's size,
// single flipped bits -- and runs the checker on each, restoring the word afterwards.  A corrupted word that is
// accepted is no defect (many words have several legal values); what the run is for is that AddressSanitizer
// and UBSan stay silent: the checker must refuse or accept, never read outside the tables or overflow.
//
// With a stride S > 1 (third argument) only the header, every S-th word and the `dense` words (fourth argument,
// default 64) behind every section's start and before it are swept: for plans whose full sweep takes too long.
// With `view` in the stride's place nothing is swept: plan_view's result is printed, every int field of PlanDev by
// name and rs_src16 -- what a change of the field list (csrc/plan_dev.h) is compared against (profiles/plan_view.txt).
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../mpc-interface_amd/csrc/plan_check.h"

using namespace mpcasm;

namespace {

template <class T>
T* read_exact(const char* path, size_t* count) {
  FILE* f = fopen(path, "rb");
  if (!f) {
    perror(path);
    exit(2);
  }
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  *count = (size_t)bytes / sizeof(T);
  T* data = static_cast<T*>(malloc(*count ? *count * sizeof(T) : 1));  // (exact size: an overrun is seen)
  if (*count && fread(data, sizeof(T), *count, f) != *count) {
    fprintf(stderr, "%s: short read\n", path);
    exit(2);
  }
  fclose(f);
  return data;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s ITAB DTAB [stride [dense] | view]\n", argv[0]);
    return 2;
  }
  size_t n = 0, nd = 0;
  int32_t* it = read_exact<int32_t>(argv[1], &n);
  double* dt = read_exact<double>(argv[2], &nd);
  const size_t stride = argc > 3 ? (size_t)atol(argv[3]) : 1, dense = argc > 4 ? (size_t)atol(argv[4]) : 64;
  if (validate_plan(it, dt, n, nd) != MPCASM_OK) {
    fprintf(stderr, "%s: the untouched tables are refused\n", argv[1]);
    return 1;
  }
  if (argc > 3 && !strcmp(argv[3], "view")) {
    PlanDev d = {};  // (rs_p_direct is not plan_view's: it stays 0)
    plan_view(it, &d);
    printf("%s: sizeof(PlanDev) %zu\n", argv[1], sizeof(PlanDev));
#define SHOW(f, ...) printf("  %s %d\n", #f, d.f);
    MPCASM_PLAN_INT_FIELDS(SHOW, SHOW)
#undef SHOW
    printf("  rs_src16 %u\n", d.rs_src16);
    free(it);
    free(dt);
    return 0;
  }
  // where sections start: every header word that can be an offset into itab
  std::vector<size_t> starts;
  for (size_t w = 0; w < (size_t)H_WORDS; ++w)
    if (it[w] >= H_WORDS && (size_t)it[w] <= n) starts.push_back((size_t)it[w]);
  starts.push_back(n);
  std::sort(starts.begin(), starts.end());
  auto swept = [&](size_t w) {
    if (stride <= 1 || w < (size_t)H_WORDS || w % stride == 0) return true;
    const auto next = std::upper_bound(starts.begin(), starts.end(), w);  // the first start behind w
    return (next != starts.end() && *next - w <= dense) || (next != starts.begin() && w - *(next - 1) < dense);
  };
  long accepted = 0, refused = 0, words = 0;
  for (size_t w = 0; w < n; ++w) {
    if (!swept(w)) continue;
    ++words;
    const int32_t old = it[w];
    const uint32_t u = (uint32_t)old;  // (candidates in unsigned arithmetic: no overflow of our own)
    const uint32_t values[] = {(uint32_t)-1, 0u, 1u, u - 1u, u + 1u, u + 2u, 2u * u, 65535u, 65536u,
                               (uint32_t)INT_MAX, (uint32_t)INT_MIN, (uint32_t)n - 1u, (uint32_t)n,
                               u ^ (1u << 8), u ^ (1u << 16), u ^ (1u << 24)};
    for (uint32_t v : values) {
      if (v == u) continue;
      it[w] = (int32_t)v;
      const int rc = validate_plan(it, dt, n, nd);
      if (rc == MPCASM_OK) {
        ++accepted;
      } else if (rc == MPCASM_ERR_PLAN || rc == MPCASM_ERR_LIMIT) {
        ++refused;
      } else {
        fprintf(stderr, "word %zu = %d: status %d\n", w, (int)v, rc);
        return 1;
      }
    }
    it[w] = old;
  }
  if (validate_plan(it, dt, n, nd) != MPCASM_OK) {
    fprintf(stderr, "%s: the restored tables are refused\n", argv[1]);
    return 1;
  }
  printf("%s: %zu words of itab, %ld swept (stride %zu): %ld corruptions accepted, %ld refused\n", argv[1], n, words,
         stride, accepted, refused);
  free(it);
  free(dt);
  return 0;
}
