// smk_slab_occ_shadow.hip -- the slice-ring kernel's instances for the eye pass of frames with shadows AND the host's opaque
// scene depth (SHD = OCC = true; smk_slab.hip), compiled as their own translation unit: the instances are most of the
// library's build time.
#define SLAB_PART 4
#include "smk_slab.hip"
