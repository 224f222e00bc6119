// smk_slab_shadow_nv20.hip -- the slice-ring kernel's instances for the eye pass of frames with shadows in the NV20 look
// (option shadow_look 1: SHD = true, NVL = true; smk_slab.hip), compiled as their own translation unit beside
// smk_slab_shadow.hip: the instances are most of the library's build time.
#define SLAB_PART 5
#include "smk_slab.hip"
