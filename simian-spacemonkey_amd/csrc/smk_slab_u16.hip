// smk_slab_u16.hip -- the u16-voxel instances (SMK_U16) of the slice-ring kernel (smk_slab.hip), compiled as their own
// translation unit as the float-voxel ones are: 8-byte voxels staged like the byte voxels, with their own corner decode.
#define SLAB_PART 6
#include "smk_slab.hip"
