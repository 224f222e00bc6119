// smk_step_stencil.h -- what the three stencil producers of the time-step ring say alike (smk_step_derive.hip,
// smk_step_merge.hip, smk_step_merge_h.hip; DESIGN.md 3b "Where an entry's refusals, fill and launch live"): the source of
// the block instances, the refusals of the arguments that several entries take, the dispatch from a run-time (source, number
// of fields) to kernel instances, and the device helpers that place a local voxel in the volume.  The parameter structs, the
// kernels and the launches stay each producer's own.  Everything here is local to the file that includes it.
#pragma once
#include <type_traits>

#include "smk_internal.h"
#include "smk_prep_device.h"

namespace {

// ---------------------------------------------------------------------------------------------- the block instances' source

// A rank's own dense block of the volume as the kernels read it: the last members of every *BlockParams
struct StencilBlockSrc {
  int bo[3];          // the block's element [0][0][0] in LOCAL voxels of the stored box (negative: the block starts before the box)
  int c0[3], c1[3];   // C, local voxels: what of the block's extent this context takes
  long long py, pz;   // elements between two rows, two slices of the block
};

void stencil_block_src(const smk_ctx *c, const smk_block *b, const SmkBlockView &V, StencilBlockSrc &S) {
  for (int a = 0; a < 3; ++a) {
    S.bo[a] = b->origin[a] - c->O[a];
    S.c0[a] = V.c0[a] - c->O[a];
    S.c1[a] = V.c1[a] - c->O[a];
  }
  S.py = V.py;
  S.pz = V.pz;
}

// ---------------------------------------------------------------------------------------------- a local voxel in the volume

// A producer's three parameter types PT: the unsharded one (N, D), a shard's (with the SmkShardBox B) and a block's (a shard's
// with the block source)
template <class PT, class = void>
constexpr bool stencil_shard = false;
template <class PT>
constexpr bool stencil_shard<PT, std::void_t<decltype(PT::B)>> = true;
template <class PT>
constexpr bool stencil_block = std::is_base_of<StencilBlockSrc, PT>::value;

// local voxel l of axis a as a voxel of the volume
template <class PT>
__device__ __forceinline__ int stencil_glob(const PT &P, int a, int l) {
  if constexpr (stencil_shard<PT>) return P.B.O[a] + l;
  else return l;
}

// local voxel (X, Y, Z) is a voxel of the volume that the source holds
template <class PT>
__device__ __forceinline__ bool stencil_held(const PT &P, int X, int Y, int Z) {
  if constexpr (stencil_block<PT>)
    return X >= P.c0[0] && X < P.c1[0] && Y >= P.c0[1] && Y < P.c1[1] && Z >= P.c0[2] && Z < P.c1[2];
  else if constexpr (stencil_shard<PT>)
    return X >= 0 && X < P.D[0] && P.B.O[0] + X < P.N[0] && Y >= 0 && Y < P.D[1] && P.B.O[1] + Y < P.N[1] && Z >= 0 && Z < P.D[2] &&
           P.B.O[2] + Z < P.N[2];
  else return X >= 0 && X < P.N[0] && Y >= 0 && Y < P.N[1] && Z >= 0 && Z < P.N[2];
}

// ---------------------------------------------------------------------------------------------- the shared refusals

// the eight words of an export, or the combined ones
int stencil_words_refusals(smk_ctx *c, const char *who, const void *d_words) {
  if (!d_words) FAIL(c, "%s: d_words is NULL", who);
  if ((uintptr_t)d_words % sizeof(int)) FAIL(c, "%s: d_words is not aligned to its 4-byte words", who);
  return 0;
}

// the kind of smk_step_extremes_device and smk_block_extremes_device
int stencil_kind_refusals(smk_ctx *c, const char *who, int kind) {
  if (kind != SMK_EXTREMES_DERIVE && kind != SMK_EXTREMES_MERGE)
    FAIL(c, "%s: kind %d is neither SMK_EXTREMES_DERIVE (%d) nor SMK_EXTREMES_MERGE (%d)", who, kind, (int)SMK_EXTREMES_DERIVE,
         (int)SMK_EXTREMES_MERGE);
  return 0;
}

// the sizes of a dense array of the whole volume against the series'; sz null (a block says itself what it holds): nothing
int stencil_sizes_refusals(smk_ctx *c, const char *who, int timestep, const int *sz) {
  if (sz && (sz[0] != c->N[0] || sz[1] != c->N[1] || sz[2] != c->N[2]))
    FAIL(c, "%s: time step %d: sizes %dx%dx%d differ from the series' %dx%dx%d", who, timestep, sz[0], sz[1], sz[2], c->N[0], c->N[1], c->N[2]);
  return 0;
}

// The derive's dense scalar: NULL, the type, (sz: the sizes,) the alignment
int stencil_scalar_refusals(smk_ctx *c, const char *who, const void *d_scalar, smk_dtype dt, int timestep, const int *sz) {
  if (!d_scalar) FAIL(c, "%s: d_scalar is NULL", who);
  if (dt != SMK_U8 && dt != SMK_U16 && dt != SMK_F32) FAIL(c, "%s: scalar_dtype %d is none of SMK_U8, SMK_U16, SMK_F32", who, (int)dt);
  if (stencil_sizes_refusals(c, who, timestep, sz)) return 1;
  const size_t eb = smk_elem_bytes(dt);
  if ((uintptr_t)d_scalar % eb) FAIL(c, "%s: d_scalar is not aligned to its %zu-byte elements", who, eb);
  return 0;
}

// The merges' dense fields: a NULL array, their number (add_h null: the merge without H, whose message does not speak of it),
// the type against the ring's, (sz: the sizes,) every field's pointer and alignment
int stencil_fields_refusals(smk_ctx *c, const char *who, const void *const *d_fields, int nf, smk_dtype dt, const int *add_h, int timestep,
                            const int *sz) {
  if (!d_fields) FAIL(c, "%s: d_fields is NULL", who);
  if (!add_h && nf != c->nelts - 1)
    FAIL(c, "%s: %d fields for a series of nelts %d: the fields are nelts - 1 = %d", who, nf, c->nelts, c->nelts - 1);
  if (add_h && nf != c->nelts - 1 - *add_h)
    FAIL(c, "%s: %d fields for a series of nelts %d with add_h %d: the fields are nelts - 1 - add_h = %d", who, nf, c->nelts, *add_h,
         c->nelts - 1 - *add_h);
  if ((int)dt != c->dtype) FAIL(c, "%s: field_dtype %d is not the ring's type (%d): the fields are stored as they come", who, (int)dt, c->dtype);
  if (stencil_sizes_refusals(c, who, timestep, sz)) return 1;
  const size_t eb = smk_elem_bytes(dt);
  for (int e = 0; e < nf; ++e) {
    if (!d_fields[e]) FAIL(c, "%s: d_fields[%d] is NULL", who, e);
    if ((uintptr_t)d_fields[e] % eb) FAIL(c, "%s: d_fields[%d] is not aligned to its %zu-byte elements", who, e, eb);
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------- the dispatch

// A kernel's SRC template argument (smk_prep_device.h): dense arrays of a type, or the packed voxels of a slot of that type
constexpr int stencil_ring(int SRC) { return SRC == SRC_PK_U8 ? SMK_U8 : SRC == SRC_PK_U16 ? SMK_U16 : SRC == SRC_PK_F32 ? SMK_F32 : SRC; }

enum { PASS_1 = 1, PASS_2 = 2 };  // what a launch function enqueues: the seed and pass 1, pass 2, or both

// f(SRC) for the source of type dt -- a packed slot (PACKED) or dense arrays --, SRC a std::integral_constant.  Only the sources
// of one kind are instantiated: a shard's kernels have no dense instance, a block's no packed one
template <bool PACKED, class F>
hipError_t stencil_dispatch_src(int dt, F &&f) {
  switch (dt) {
    case SMK_U8: return f(std::integral_constant<int, PACKED ? (int)SRC_PK_U8 : (int)SMK_U8>());
    case SMK_U16: return f(std::integral_constant<int, PACKED ? (int)SRC_PK_U16 : (int)SMK_U16>());
    case SMK_F32: return f(std::integral_constant<int, PACKED ? (int)SRC_PK_F32 : (int)SMK_F32>());
  }
  return hipErrorInvalidValue;
}

// ... and f(SRC, NF) for nf fields besides: 1 to 3, and no third of 16-bit voxels, which hold three channels
template <bool PACKED, class F>
hipError_t stencil_dispatch(int dt, int nf, F &&f) {
  return stencil_dispatch_src<PACKED>(dt, [&](auto src) -> hipError_t {
    if (nf == 1) return f(src, std::integral_constant<int, 1>());
    if (nf == 2) return f(src, std::integral_constant<int, 2>());
    if constexpr (stencil_ring(decltype(src)::value) != SMK_U16) {
      if (nf == 3) return f(src, std::integral_constant<int, 3>());
    }
    return hipErrorInvalidValue;
  });
}

}  // namespace
