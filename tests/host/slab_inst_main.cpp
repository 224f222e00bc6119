// slab_inst_main.cpp -- the instance table of the slice-ring kernel as the library's own header states it (smk_slab.h
// slab_inst_missing / slab_inst_part), one line per key of the full cross product:
//   dt sh perm nw nl diag tf br shd occ nvl  (the order of smk_k_slab's template arguments), then "built <part>" or the reason
// No device, no library: the header's host side only.  tests/test_slab_instances_cpu.py compares it with the kernels that
// libsmk_hip.so holds.
#include <cstdio>

#include "../../simian-spacemonkey_amd/csrc/smk_slab.h"

int main() {
  for (int i = 0; i < SLAB_INST_KINDS; ++i)
    for (int f = 0; f < SLAB_INST_FLAGS; ++f) {
      const SlabInst k = slab_inst_at(i, f);
      printf("%d %d %d %d %d %d %d %d %d %d %d ", k.dt, k.sh, k.perm, k.nw, k.nl, (int)k.diag, k.tf, (int)k.br, (int)k.shd, (int)k.occ, (int)k.nvl);
      if (const char *why = slab_inst_missing(k))
        printf("%s\n", why);
      else
        printf("built %d\n", slab_inst_part(k));
    }
  return 0;
}
