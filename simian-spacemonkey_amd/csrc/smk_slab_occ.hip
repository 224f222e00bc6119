// smk_slab_occ.hip -- the slice-ring kernel's instances for frames with the host's opaque scene depth (OCC = true,
// smk_render_occluded; smk_slab.hip), both voxel types, compiled as their own translation unit: the instances are most of
// the library's build time.
#define SLAB_PART 3
#include "smk_slab.hip"
