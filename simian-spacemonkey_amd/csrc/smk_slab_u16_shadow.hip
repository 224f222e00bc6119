// smk_slab_u16_shadow.hip -- the u16-voxel instances of the slice-ring kernel for the eye pass of frames with shadows
// under look 0 (smk_slab.hip, SHD instances), in a translation unit of their own.
#define SLAB_PART 7
#include "smk_slab.hip"
