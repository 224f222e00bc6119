// smk_step_block.hip -- a time step from a rank's own dense block of the volume, the packed form (smk.h: smk_block,
// smk_upload_timestep_block_device; DESIGN.md 3b "Blocks of a decomposed simulation"), and the data-free fill of
// smk_declare_volume.
//
// smk_upload_timestep_device packs bricks that tile the whole volume, each a contiguous array (smk_k_pack, smk_api.hip: a
// thread per SOURCE voxel).  A block is one pitched array that covers a part of the stored box; the rest of the box has to be
// written too, because a ring slot keeps what the step before left there.  So the kernel here runs a thread per STORED voxel
// and writes the whole box in one pass: inside C the voxel smk_k_pack would store -- the same smk_packed.h expressions on the
// same values, read through the block's pitches --, on the rim zeros with the normal (128, 128, 128), in the pad column and
// row zeros.  The stencil forms of a block are instances of the tiled kernels (smk_step_derive.hip, smk_step_merge.hip).
#include "smk_internal.h"

namespace {

struct PackBlockParams {
  const void *src;            // the block's [z][y][x][nelts] elements, or null: no voxel lies in C
  const unsigned char *grad;  // its [z][y][x][3] normals, or null
  void *dst;                  // the slot's packed voxels
  uint32_t *nrm;              // its separate normal words (four-channel f32 with normals), else null
  int N[3], O[3], D[3];
  int bo[3], c0[3], c1[3];    // LOCAL voxels of the stored box: the block's element [0][0][0]; C
  long long py, pz;           // elements between two rows, two slices of the block
  int nelts, n_in_w;
};

template <int DT>
__global__ __launch_bounds__(256) void smk_k_pack_block(const PackBlockParams P) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, row = (size_t)P.D[0], slice = row * P.D[1];
  if (t >= slice * P.D[2]) return;
  const int Z = (int)(t / slice), Y = (int)((t - (size_t)Z * slice) / row), X = (int)(t - (size_t)Z * slice - (size_t)Y * row);
  if (DT != SMK_F32 && (P.O[0] + X >= P.N[0] || P.O[1] + Y >= P.N[1])) {  // the pad column or row of an 8-byte box: zeros, as after an upload
    ((uint2 *)P.dst)[t] = make_uint2(0u, 0u);
    return;
  }
  const bool in = P.src && X >= P.c0[0] && X < P.c1[0] && Y >= P.c0[1] && Y < P.c1[1] && Z >= P.c0[2] && Z < P.c1[2];
  if (!in) {  // the rim: zeros that carry no normal
    if (DT == SMK_F32) {
      ((uint4 *)P.dst)[t] = make_uint4(0u, 0u, 0u, P.n_in_w ? SMK_NRM_NONE : 0u);
      if (P.nrm) P.nrm[t] = SMK_NRM_NONE;
    } else {
      ((uint2 *)P.dst)[t] = make_uint2(0u, SMK_NRM_NONE);
    }
    return;
  }
  const size_t e = (size_t)(Z - P.bo[2]) * (size_t)P.pz + (size_t)(Y - P.bo[1]) * (size_t)P.py + (size_t)(X - P.bo[0]);
  uint32_t nb = SMK_NRM_NONE;
  if (P.grad) nb = smk_nrm_word(P.grad[e * 3], P.grad[e * 3 + 1], P.grad[e * 3 + 2]);
  if (DT == SMK_U8) {
    ((uint2 *)P.dst)[t] = smk_pack_u8((const unsigned char *)P.src + e * P.nelts, P.nelts, nb);
  } else if (DT == SMK_U16) {
    ((uint2 *)P.dst)[t] = smk_pack_u16((const unsigned short *)P.src + e * P.nelts, P.nelts, nb);
  } else {
    const uint4 v = smk_pack_f32((const float *)P.src + e * P.nelts, P.nelts, nb, P.n_in_w);
    if (!P.n_in_w && P.nrm) P.nrm[t] = nb;
    ((uint4 *)P.dst)[t] = v;
  }
}

}  // namespace

hipError_t smk_pack_block(const smk_ctx *c, const void *src, const unsigned char *grad, const int bo[3], const int c0[3], const int c1[3],
                          long long py, long long pz, TimeStep &T, hipStream_t s) {
  PackBlockParams P;
  P.src = src;
  P.grad = grad;
  P.dst = T.vox;
  P.nrm = smk_step_separate_normals(c) ? T.nrm : nullptr;
  for (int a = 0; a < 3; ++a) {
    P.N[a] = c->N[a];
    P.O[a] = c->O[a];
    P.D[a] = c->D[a];
    P.bo[a] = bo[a];
    P.c0[a] = c0[a];
    P.c1[a] = c1[a];
  }
  P.py = py;
  P.pz = pz;
  P.nelts = c->nelts;
  P.n_in_w = c->dtype == SMK_F32 && c->nelts <= 3 ? 1 : 0;
  const size_t total = (size_t)c->D[0] * c->D[1] * c->D[2], blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;  // (2^39 stored voxels: no device holds such a box)
  if (c->dtype == SMK_U8) hipLaunchKernelGGL(smk_k_pack_block<SMK_U8>, dim3((unsigned)blocks), dim3(256), 0, s, P);
  else if (c->dtype == SMK_U16) hipLaunchKernelGGL(smk_k_pack_block<SMK_U16>, dim3((unsigned)blocks), dim3(256), 0, s, P);
  else hipLaunchKernelGGL(smk_k_pack_block<SMK_F32>, dim3((unsigned)blocks), dim3(256), 0, s, P);
  return hipGetLastError();
}

extern "C" int smk_upload_timestep_block_device(smk_ctx *c, int timestep, const void *d_data, const unsigned char *d_grad, const smk_block *b,
                                                void *stream) {
  if (!c) return 1;
  const char *who = "smk_upload_timestep_block_device";
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_volume) FAIL(c, "%s: no volume uploaded (smk_declare_volume gives a context its geometry without data)", who);
  if (timestep < 0) FAIL(c, "%s: time step %d: ids are >= 0", who, timestep);
  if (!d_data) FAIL(c, "%s: d_data is NULL", who);
  const size_t eb = smk_elem_bytes(c->dtype);
  if ((uintptr_t)d_data % eb) FAIL(c, "%s: d_data is not aligned to its %zu-byte elements", who, eb);
  if ((d_grad != nullptr) != c->have_normals)
    FAIL(c, "%s: time step %d: normals %s, the series' %s", who, timestep, d_grad ? "present" : "absent", c->have_normals ? "present" : "absent");
  SmkBlockView V;
  if (smk_block_view(c, who, b, V)) return 1;
  if (c->nranks > 1 && V.halo < 1)
    FAIL(c, "%s: the block gives a valid halo of %d voxels: a frame's trilinear fetch needs a valid halo >= 1", who, V.halo);
  const hipStream_t s = stream ? (hipStream_t)stream : c->stream;
  return smk_step_produce(c, who, timestep, -1, -1, s, [&](TimeStep &T, const TimeStep *, const TimeStep *) -> int {
    SmkShardBox B;
    smk_step_block_box(c, V, 0, B);
    int bo[3];
    for (int a = 0; a < 3; ++a) bo[a] = b->origin[a] - c->O[a];
    HIPCHK(c, smk_pack_block(c, d_data, d_grad, bo, B.v0, B.v1, V.py, V.pz, T, s));
    smk_step_block_done(c, V, 0, B, T);
    return 0;
  });
}
