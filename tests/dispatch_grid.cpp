// dispatch_grid.cpp — prints the decisions of pbd_dispatch.h over a grid, for
// tests/test_dispatch.py (plain host C++, no HIP):
//   kind L feat gw env fold <step> <policy> <eval_policy> <eval_open> <population>
//     per family the env kind's own kernel F/M/EK, or - for the variant list
//   wide workgroups tpb cus 0|1
//   step_kernel F/M/EK|- step|packed|rollout narrow|wide <kernel name>
//   bad ...   a decision that is not in its list of instantiations
#include <stdio.h>

#include <set>
#include <string>

#include "../brax_amd/csrc/pbd_dispatch.h"
#include "../include/brax_amd.h"

using namespace bx;

static std::string show(KindVariant v) {
  if (v.EK == EK_ANY) return "-";
  char b[64];
  snprintf(b, sizeof b, "%d/%d/%d", v.F, v.M, v.EK);
  return b;
}
static bool kind_listed(KindVariant v) {
#define LISTED(VF, VM, VEK, UNUSED) \
  if (v.F == (VF) && v.M == (VM) && v.EK == (VEK)) return true;
  BX_KIND_VARIANTS(LISTED, 0)
#undef LISTED
  return false;
}
static bool single_listed(SingleVariant v) {
#define LISTED(VL, VF, VM, UNUSED) \
  if (v.L == (VL) && v.F == (VF) && v.M == (VM)) return true;
  BX_SINGLE_VARIANTS(LISTED, 0)
#undef LISTED
  return false;
}

int main() {
  std::set<int> feats;
#define ADD(VL, VF, VM, UNUSED) feats.insert(VF);
  BX_SINGLE16_VARIANTS(ADD, 4, 0)
#undef ADD
  for (int m : {(int)F_ENV_ANT, (int)F_ENV_HUM, (int)F_ENV_CHEETAH, (int)F_ENV_PUSHER, (int)F_ENV_STANDUP}) {
    feats.insert(m | F_G1);
    feats.insert(m & ~F_G1);
  }
  const struct {
    int kind;
    const char* name;
  } kinds[] = {{BX_ENV_ANT, "ant"}, {BX_ENV_HUMANOID, "humanoid"},
               {BX_ENV_HUMANOID_STANDUP, "humanoidstandup"}, {BX_ENV_HALFCHEETAH, "halfcheetah"},
               {BX_ENV_PUSHER, "pusher"}, {BX_ENV_HOPPER, "hopper"}};
  const EnvFamily fams[] = {FAM_STEP, FAM_POLICY, FAM_EVAL_POLICY, FAM_EVAL_OPEN, FAM_POPULATION};
  for (int L : {16, 32, 64})
    for (int feat : feats)
      for (int gw : {4, 8}) {
        const SingleVariant sv = single_variant(L, feat, gw);
        if (!single_listed(sv)) printf("bad single %d %d %d -> %d %d %d\n", L, feat, gw, sv.L, sv.F, sv.M);
        for (const auto& k : kinds)
          for (int fold : {0, 1, 3, 5, 7}) {
            printf("kind %d %d %d %s %d", L, feat, gw, k.name, fold);
            for (EnvFamily fam : fams) {
              const KindVariant v = kind_variant(fam, L, feat, gw, k.kind, fold);
              if (v.EK != EK_ANY && (!kind_listed(v) || !family_has(fam, v.EK)))
                printf(" bad");
              printf(" %s", show(v).c_str());
            }
            printf("\n");
          }
      }
  // fold_bits composes the grid's fold values
  if (fold_bits(false, true, true) != 0 || fold_bits(true, false, false) != 1 ||
      fold_bits(true, true, false) != 3 || fold_bits(true, false, true) != 5 ||
      fold_bits(true, true, true) != 7)
    printf("bad fold_bits\n");
  for (int cus : {256, 304})
    for (int tpb : {32, 64})
      for (int d = -1; d <= 1; d++)
        printf("wide %d %d %d %d\n", 4 * cus + d, tpb, cus, (int)ant_wide(4 * cus + d, tpb, cus));
  // the step family's kernel per instantiation, launch form and batch width
  const char* names[] = {"env_step_kernel", "env_step_packed_kernel", "env_rollout_kernel",
                         "env_step_wide_kernel", "env_rollout_wide_kernel"};
  const struct {
    int n_steps;
    bool packed;
    const char* name;
  } forms[] = {{1, false, "step"}, {1, true, "packed"}, {5, true, "rollout"}};
  auto step_rows = [&](KindVariant v) {
    for (const auto& f : forms)
      for (int w = 0; w < 2; w++)
        printf("step_kernel %s %s %s %s\n", show(v).c_str(), f.name, w ? "wide" : "narrow",
               names[step_kernel(v, w != 0, f.n_steps, f.packed)]);
  };
#define ROWS(VF, VM, VEK, UNUSED) step_rows(KindVariant{VF, VM, VEK});
  BX_KIND_VARIANTS(ROWS, 0)
#undef ROWS
  step_rows(KindVariant{0, 0, EK_ANY});
  return 0;
}
