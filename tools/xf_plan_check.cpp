// gill_amd/csrc/xf_plan.h on its own, for a host sanitizer run (it is plain C++: no HIP header, no library):
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -I gill_amd/csrc tools/xf_plan_check.cpp -o /tmp/xf_plan_check
//   python tools/xf_plan_check.py | /tmp/xf_plan_check
// stdin: one case per line, `lnproj xalg ffn_fused  C heads ctx_len ctx_dim hw fp8 Bx shared  <the 11 expected ints>` (tools/xf_plan_check.py prints the
// table of tests/test_xf_plan_host.py in this form); every line goes through xf_forms() / xf_forms_consistent() / xf_plan() and is compared.
// The two shape predicates live beside their kernels (ffn.hip, lnproj.hip) and the padded head dim in ops.h; they are restated here so that this
// program links alone — the comparison with the table (which the library also has to meet) is what keeps the three honest.
#include <stdio.h>
#include <string.h>
#include "xf_plan.h"

bool ffn_fused_supported(int C, int M) { return C == 320 && M % 128 == 0 && M > 0; }
bool lnproj_supported(int C, int M, int heads, int dp) { return C == 320 && M > 0 && M % 128 == 0 && heads == 8 && dp == 48; }
static int padded_head_dim(int d) { return d <= 48 ? 48 : d <= 64 ? 64 : d <= 80 ? 80 : d <= 128 ? 128 : d <= 160 ? 160 : 0; }

int main() {
  int v[22], n = 0, bad = 0;
  for (;;) {
    int got = 0;
    for (int& x : v) got += scanf("%d", &x) == 1;
    if (got == 0) break;
    if (got != 22) { fprintf(stderr, "case %d: short line\n", n); return 2; }
    const XfEnv env = {v[0] != 0, v[1] != 0, v[2] != 0};
    const XfGeom g = {v[3], v[4], padded_head_dim(v[3] / v[4]), v[5], v[6], v[7], v[8]};
    const XfForms f = xf_forms(g, env);
    const XfPlan p = xf_plan(f, g, v[9], v[7], v[10] != 0);
    int row[11];
    memcpy(row, &f, sizeof f);
    memcpy(row + 5, &p, sizeof p);
    static_assert(sizeof f == 5 * sizeof(int) && sizeof p == 6 * sizeof(int), "a row is 5 + 6 ints");
    if (!xf_forms_consistent(f) || memcmp(row, v + 11, sizeof row) != 0) {
      ++bad;
      fprintf(stderr, "case %d differs:", n);
      for (int x : row) fprintf(stderr, " %d", x);
      fprintf(stderr, "\n");
    }
    ++n;
  }
  const XfEnv& e = xf_env_default();
  printf("%d cases, %d differ; environment switches: lnproj %d xalg %d ffn_fused %d\n", n, bad, e.lnproj, e.xalg, e.ffn_fused);
  return bad != 0 || n == 0;
}
