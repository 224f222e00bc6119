/*
 * smk.h -- C ABI of the MI355X-native volume ray-marcher that takes over Simian's renderer slot.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  A
 * gluvvPrimitive subclass (INTEGRATION.md shows it; a buildable mirror lives in
 * simian-spacemonkey_amd/host/) calls these from init()/draw() instead of issuing OpenGL.
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference tree, zzmuxi/simian-spacemonkey).
 *
 * Conventions (VolumeRenderer.cpp:101-126, glUE.cpp:194-207): int returns are 0 = ok,
 * non-zero = error, message via smk_last_error(); nothing throws.  Inputs are copied at the
 * call (the reference renderers copy into texture memory at init(), NV20VolRen3D.cpp:1315-1330);
 * the caller keeps ownership of every pointer it passes.  One context per GPU, not thread-safe
 * (the reference is single-threaded GLUT).  There is NO CPU fallback: without a HIP device
 * smk_create() fails.
 */
#ifndef SMK_H
#define SMK_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct smk_ctx smk_ctx;

/* voxel storage handed over by the caller.
 * SMK_U16: [z][y][x][nelts] uint16_t in host byte order, nelts 1..3 (4 is refused: "4-channel u16 voxels"), for the 12 to
 * 16-bit integer data of CT, MR and most instruments.  The reference quantises such bricks to bytes (MetaVolume.cpp:709-889,
 * quantize<T>); here they are stored in the 8 bytes of a u8 voxel,
 *     uint2 { c0 | c1 << 16,   n0 | n1 << 8 | n2 << 16 | q8(c2) << 24 },   q8(c) = (c * 255 + 32767) / 65535,
 * so channels 0 and 1 -- the two axes of the 2-D table -- keep all 16 bits, and channel 2 (the second derivative / third
 * table axis of the VGH modes) is kept at the nearest 8-bit unorm: THAT IS THE LIMIT OF THE TYPE.  A missing channel is 0,
 * missing normals are (128, 128, 128).  A sample interpolates the raw integers as floats and scales once:
 * ch0 = T0 / 65535, ch1 = T1 / 65535, ch2 = T2 / 255; everything after the channel values is the u8 / f32 code.  Normals are
 * [z][y][x][3] u8 as for the other types.  Everything a u8 volume does, it does: bricked and shuffled uploads, shards, time
 * steps (a ring is of one type: a step of another dtype is refused, as a changed geometry is), brick flags, all data modes
 * of at most three channels, perturbation, shadows under the two marches in both looks, smk_render_slice, the clip-plane
 * widget's slice, smk_count_samples.  The gather kernel renders every such frame; the slice-ring kernel has the plain
 * instances and the eye pass of frames with shadows under look 0 -- bit-identical frames -- and declines, with the reason,
 * frames with the host's scene depth, the NV20 look, and NV20 shading under the 3-D table with brick flags on its 10+2-wave
 * shapes (those instances would need scratch): auto mode then renders on the gather kernel, a forced "kernel" 2 fails.
 * Refused with the reason: the column-stream kernel ("kernel" 3), shadows with option "shadow_march" 0 or "shadow_fused". */
typedef enum { SMK_U8 = 0, SMK_F32 = 1, SMK_U16 = 2 } smk_dtype;

/* gluvvDataMode, same order and meaning (gluvv.h:221-235) */
typedef enum {
  SMK_GDM_V1, SMK_GDM_V1G, SMK_GDM_V1GH, SMK_GDM_V2, SMK_GDM_V2G, SMK_GDM_V2GH, SMK_GDM_V3,
  SMK_GDM_V3G, SMK_GDM_V4, SMK_GDM_VGH, SMK_GDM_VGH_VG, SMK_GDM_VGH_V, SMK_GDM_UNKNOWN
} smk_datamode;

/* shading: gluvvShade (gluvv.h:199-207) collapsed to what the two VGH renderers implement */
typedef enum {
  SMK_SHADE_NONE = 0,      /* gluvvShadeAmb / Faux: colour * alpha only                        */
  SMK_SHADE_R8K_DIFF = 1,  /* R8kVolRen3D cube-map Phong, diffuse only (gluvvShadeDiff)         */
  SMK_SHADE_R8K_DSPEC = 2, /* R8kVolRen3D diffuse + specular^30 (gluvvShadeDSpec) -- canonical  */
  SMK_SHADE_NV20_DIFF = 3, /* NV20VolRen3D register-combiner Phong, diffuse                     */
  SMK_SHADE_NV20_DSPEC = 4 /* NV20VolRen3D diffuse + specular^16                                */
} smk_shade;

/* framebuffer blend of the slice polygons (SURVEY 2.1 "Framebuffer blend") */
typedef enum {
  SMK_BLEND_FRONT_TO_BACK = 0, /* GL_ONE_MINUS_DST_ALPHA, GL_ONE (R8kVolRen3D.cpp:1441-1449); exact early termination */
  SMK_BLEND_BACK_TO_FRONT = 1, /* GL_ONE, GL_ONE_MINUS_SRC_ALPHA, far plane first (VolumeRenderer.cpp:590, NV20VolRen3D.cpp:930) */
  SMK_BLEND_MAX = 2            /* glBlendEquationEXT(GL_MAX): gluvvShadeMIP (NV20VolRen3D.cpp:158-163) */
} smk_blend;

/* Exactly the fields of `class Volume` a renderer reads (MetaVolume.h:18-61): one brick as
 * produced by MetaVolume::brick (MetaVolume.cpp:1369-1452). */
typedef struct {
  int xiSize, yiSize, ziSize;   /* voxels                                                  */
  float xfSize, yfSize, zfSize; /* extent in volume space                                  */
  int xiPos, yiPos, ziPos;      /* voxel origin inside the whole volume                    */
  float xfPos, yfPos, zfPos;    /* origin in volume space                                  */
  const void *data;             /* currentData: [z][y][x][nelts], u8, f32 or u16           */
  const unsigned char *grad;    /* currentGrad: [z][y][x][3] scale-biased normals, or NULL */
} smk_volume_desc;

/* replaces `new VolumeRenderer(gluvv.mv,0)` / the renderer constructors (VolumeRenderable.cpp:66,
 * gluvv.cpp:141-199).  device_ordinal >= 0.  *err (may be NULL) gets 0 or an error code. */
smk_ctx *smk_create(int device_ordinal, int *err);
void smk_destroy(smk_ctx *ctx);
const char *smk_last_error(smk_ctx *ctx); /* ctx may be NULL: last smk_create failure */

/* replaces VolumeRenderer::createVolume x2 (VolumeRenderer.cpp:101-212) and
 * NV20VolRen3D/R8kVolRen3D::createBricks (NV20VolRen3D.cpp:1255-1369, R8kVolRen3D.cpp:1926-2055):
 * copies the bricks of one MetaVolume into HBM.  Bricks must tile the volume (MetaVolume::brick
 * output, or a single whole volume).  They are re-assembled into one dense volume with global
 * voxel addressing, which removes the reference's seam artefacts. */
int smk_upload_volume(smk_ctx *ctx, const smk_volume_desc *bricks, int n_bricks, int nelts,
                      smk_dtype dtype, smk_datamode dmode);
/* same, but data/grad are DEVICE pointers on this context's GPU (volumes produced on the GPU,
 * e.g. by smk_synth_volume/smk_make_vgh_device; no PCIe copy) */
int smk_upload_volume_device(smk_ctx *ctx, const smk_volume_desc *bricks, int n_bricks, int nelts,
                             smk_dtype dtype, smk_datamode dmode);

/* ---- time-varying data sets: a ring of time steps resident in device memory (DESIGN.md "Time steps").  The reference
 * keeps `tstepCache` steps of a series in host memory (MetaVolume::swapTStep / cacheTStep, MetaVolume.cpp:894-958) and
 * rebuilds its textures when gluvv.volren.timestep moves (R8kVolRen3D.cpp:184-188, keys +/- gluvv.cpp:970-1010).  A step is
 * what smk_upload_volume makes of a volume (packed voxels, normals, brick summaries; on a shard its region + halo); a switch
 * copies no voxel.  Time-step ids are >= 0.  smk_upload_volume[_device] drops every cached step and stores its volume as the
 * current step (id 0 on a new context, else the current id); a context that never calls these renders exactly as before. */
/* replaces MetaVolume::tstepCache: how many steps stay resident (default 1: the current one).  Shrinking frees the steps that
 * were written longest ago (never the current one); a capacity whose new steps do not fit in free device memory is refused,
 * with the bytes per step (an x-major copy, made for views along x, adds as much again as the voxels). */
int smk_set_timestep_cache(smk_ctx *ctx, int nsteps);
/* replaces MetaVolume::readAll + cacheTStep (MetaVolume.cpp:894-958): stores one step without changing the current one
 * (on a context without a volume the first step stored becomes current).  A step cached under that id is overwritten in
 * place; otherwise the step takes an empty slot, else the slot after the one written last -- never the current step's (with
 * a capacity of 1 the call is refused).  The bricks as for smk_upload_volume, with the first upload's geometry: sizes,
 * extents, nelts, dtype, datamode, normals present or not (a mismatch is refused, the field named).  Synchronous. */
int smk_upload_timestep(smk_ctx *ctx, int timestep, const smk_volume_desc *bricks, int n_bricks, int nelts, smk_dtype dtype,
                        smk_datamode dmode);
/* same with DEVICE data/grad pointers, asynchronous on `stream` (a hipStream_t, NULL = the context's stream): the pack and
 * the brick summaries are enqueued there behind the last frame that read the slot, and the frames that render the step wait
 * for them on their own streams.  The caller keeps the bricks alive until `stream` has passed the upload. */
int smk_upload_timestep_device(smk_ctx *ctx, int timestep, const smk_volume_desc *bricks, int n_bricks, int nelts,
                               smk_dtype dtype, smk_datamode dmode, void *stream);
/* replaces MetaVolume::swapTStep: the next frame renders that step.  A step that is not cached fails with "not cached"
 * (swapTStep's return 0): the host uploads it (smk_upload_timestep) and selects it again. */
int smk_select_timestep(smk_ctx *ctx, int timestep);
/* Fractional time (no reference counterpart: swapTStep swaps whole steps).  Step `step_out` becomes the blend
 * (1 - w) a + w b of the cached steps `step_a` and `step_b`, field by field of the packed voxels, in a slot of the ring as if
 * it had been uploaded: smk_select_timestep(step_out) shows it, smk_get_timesteps lists it, every kernel, option and shard
 * renders it like any step.  It does not become current unless it already was.
 * Arithmetic (the contract; plain fp32, one rounding per operation, in the order written):
 *   u = 1.0f - w, once;  for the values x of a and y of b of every stored field:  r = (u * x) + (w * y)
 *   -- two products and one sum, never an fma.  A float channel stores r (non-finite inputs give what this arithmetic
 *   gives, and the brick summary flags their brick as after an upload); an integer field stores
 *   min((int)(r + 0.5f), top), top = 255 for bytes, 65535 for 16-bit channels.  The fields: u8 -- the four channel bytes and
 *   the three normal bytes; u16 -- channels 0 and 1 as 16-bit values, the three normal bytes and the stored 8-bit third
 *   channel as bytes; f32 -- the float channels and the three normal bytes (in the separate normals buffer with four
 *   channels, when there are normals).  A missing normal is (128, 128, 128) in both steps and stays so.  w == 0 reproduces
 *   a bit for bit and w == 1 b (every integer field, every finite float); a == b is allowed and yields a copy (every integer
 *   field exactly; a float within 2.5 * 2^-24 of itself, as u + w need not be 1).
 * Normals are NOT normalised again: a blend in time shortens them as the trilinear fetch does in space.  G and H of a blend
 * are the blends of G and H, not derivatives of the blended scalar: a host that wants those blends scalars, reads the
 * blended scalar back with smk_download_timestep_device, runs the data-preparation entries (smk_make_vgh_device,
 * smk_normals_*_device, smk_merge_fields_*_device) on that array and uploads the result as another step
 * (smk_upload_timestep_device) -- all on the device ("Derivatives of a blend"); smk_derive_timestep
 * below is that recipe as one asynchronous call inside the ring.
 * Refused, with the reason: no volume; step_a or step_b not cached; step_out < 0; step_out equal to step_a or step_b (there
 * is no in-place form); w not finite or outside [0, 1]; no slot for the output.  A cached step_out is overwritten in place,
 * as by an upload (the current step too: the next frame shows the blend); otherwise it takes a slot by smk_upload_timestep's
 * rule that is not the current step's, a's or b's -- three slots, four when the current step is a fourth.
 * Asynchronous, as smk_upload_timestep_device: the blend and the brick summaries are enqueued on `stream` (NULL = the
 * context's) behind the uploads of a and b, the last frame that read the output slot and whatever still writes it; frames
 * that render the step wait for it on their own streams, and a later upload or blend into slot a or b waits for this one's
 * reads.  No host synchronisation. */
int smk_blend_timesteps(smk_ctx *ctx, int step_a, int step_b, float w, int step_out, void *stream);
/* Derivatives of a step (no reference counterpart: genVGH and MetaVolume::normalsVGH run on the host before the renderer
 * starts).  Step `step_out` becomes the VGH step of channel 0 of the cached step `step_src`: with s the stored channel 0 of
 * step_src over the whole volume (the u8 byte, the 16-bit value, or the float), the output's stored fields are exactly those
 * that smk_upload_timestep_device packs from what the data-preparation entries make of s -- the recipe of INTEGRATION.md 5,
 * bit for bit:
 *   ring SMK_U8 : channels vgh_u8 = smk_make_vgh_device(s, its type, compat); normals smk_normals_vgh_device(vgh_u8, 3, blur)
 *   ring SMK_F32: channels vgh_f32 of the same call; normals smk_normals_f32_device(vgh_f32, 3, blur)
 *   ring SMK_U16: channels smk_quantize_u16_device(vgh_f32), the third then stored as the pack's 8-bit field; normals
 *                 smk_normals_f32_device(vgh_f32, 3, blur), from the floats BEFORE quantisation
 * So: channel 0 of the output is makeVGH's RESCALED V, the affine map of the step's own interior min/max onto 0..255, not a
 * copy of the source; the 1-voxel border of the volume is 0 in all three channels; the normals' source is that output V
 * channel, border zeros included, not the input scalar; H is NaN where the gradient vanishes, and the entries' rules apply
 * (a NaN never wins an extreme, the byte cast gives 0, the float H is 0); non-finite gradients in the f32 normals give
 * (128, 128, 128); a context without normals keeps (128, 128, 128).  The pad column of a padded 8-byte box holds zeros, as
 * after an upload; the 16 bytes behind the box are not touched; the brick summaries are made for the result.
 * Refused, with the reason: no volume; a sharded context (the stencil reaches 2 voxels beyond a voxel and the scaling needs
 * the whole volume's extremes: neither fits region + halo); nelts != 3; a volume thinner than 3 voxels; step_src not cached;
 * step_out < 0; step_out == step_src (the stencil has no in-place form); no slot for the output.  A refused call changes
 * nothing.  A cached step_out is overwritten in place (the current step too); otherwise it takes a slot by
 * smk_upload_timestep's rule that is neither the source's nor the current step's -- two slots, three when the current step
 * is a third.
 * Asynchronous, ordered exactly as smk_blend_timesteps: everything is enqueued on `stream` (NULL = the context's) behind the
 * source's upload or blend and its last reader's, and behind the output slot's last frame, reader and writer; the output's
 * readiness is recorded there, and what overwrites the source later waits for this read.  No host synchronisation, no
 * device-to-host copy: the six extremes stay in a few device words that belong to the OUTPUT slot, seeded on the stream. */
int smk_derive_timestep(smk_ctx *ctx, int step_src, int step_out, int compat, int blur, void *stream);
/* The same from a dense scalar [sz][sy][sx] in DEVICE memory -- the whole volume; scalar_dtype any of SMK_U8, SMK_U16,
 * SMK_F32, whatever the ring's type -- into step `timestep`, by smk_upload_timestep_device's slot rule.  `stream` must also
 * order the reads of d_scalar.  Refused in addition: d_scalar NULL or below its element's alignment; a scalar_dtype outside
 * the three; sizes that are not the series'. */
int smk_upload_timestep_scalar_device(smk_ctx *ctx, int timestep, const void *d_scalar, smk_dtype scalar_dtype, int sx, int sy,
                                      int sz, int compat, int blur, void *stream);
/* Merged fields of a step (MetaVolume::mergeMV with addG, MetaVolume.cpp:1109-1268, which the host runs before the renderer
 * starts: the data modes SMK_GDM_V1G, _V2G, _V3G).  With nf = nelts - 1, step `step_out` becomes the multi-field step of the
 * first nf stored channels of the cached step `step_src`: its stored fields are exactly those that smk_upload_timestep_device
 * packs from what the existing merge entries make of the fields, bit for bit:
 *   ring SMK_U8 : smk_merge_fields_device(fields, nf).  Channels 0..nf-1 are the fields' bytes; channel nf is GMag's byte,
 *                 (uchar)(mag / max * 255.0) with a float quotient and a double product, 0 where the cast is out of range or
 *                 the quotient is NaN (everywhere when the maximum is 0); the normals are that entry's.
 *   ring SMK_F32: smk_merge_fields_f32_device(fields, nf).  The fields travel as raw words, NaN payloads and -0 included;
 *                 channel nf is mag / maxm, 0 where mag is not finite or maxm is 0; maxm is taken over finite magnitudes only;
 *                 a non-finite gradient gives the normal (128, 128, 128).  With nelts == 4 the normals go to the slot's
 *                 separate normals buffer.
 *   ring SMK_U16: (no merge entry exists for u16; this defines the result.)  The fields keep their stored 16-bit values.  With
 *                 F = (float)v of each field value, unscaled, smk_merge_fields_f32_device(F, nf) gives G as a float in [0, 1]
 *                 and the normals; channel nf is smk_quantize_u16_device of that G, with nf == 2 then stored as the pack's
 *                 8-bit field; the normals are the float entry's, made from the floats before any quantisation.
 * The summed gradient is g[axis] = 0.f; g[axis] += (plus - minus), fields ascending: one fp32 subtraction and one add per
 * field and axis; it is 0 on the volume's 1-voxel border.  The fields on the border are COPIED, not zeroed (smk_derive_timestep
 * zeroes them).  A context without normals keeps (128, 128, 128).  The pad column and row of a padded 8-byte box hold zeros,
 * as after an upload; the 16 bytes behind the box are not touched; the brick summaries are made for the result.  The series'
 * data mode is not looked at: the caller says whether a three-channel step is V, G, H (smk_derive_timestep) or two fields and
 * G (this entry).
 * Refused, with the reason, changing nothing: no volume; a sharded context (the stencil reaches 1 voxel beyond region + halo,
 * and the maximum is the whole volume's); nelts < 2; a volume thinner than 3 voxels; step_src not cached; step_out < 0;
 * step_out == step_src; no slot for the output.  Slots and ordering are smk_derive_timestep's: a cached step_out is
 * overwritten in place (the current step too), otherwise the output takes a slot that is neither the source's nor the current
 * step's; everything is enqueued on `stream` (NULL = the context's); no host synchronisation, no device-to-host copy, no
 * allocation: the maximum stays in a device word that belongs to the OUTPUT slot, seeded on the stream. */
int smk_merge_timestep(smk_ctx *ctx, int step_src, int step_out, void *stream);
/* The same from nf dense scalars [sz][sy][sx] in DEVICE memory, one array per field as a simulation holds them: d_fields is a
 * HOST array of nf device pointers, read before the call returns.  The fields' type is the ring's.  Into step `timestep`, by
 * smk_upload_timestep_device's slot rule; `stream` must also order the reads of the fields.  Refused in addition: d_fields
 * NULL, or any of its pointers NULL or below its element's alignment; nf != nelts - 1; field_dtype not the ring's type; sizes
 * that are not the series'. */
int smk_upload_timestep_fields_device(smk_ctx *ctx, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                      int sx, int sy, int sz, void *stream);
/* Merged fields of a step WITH H and blurred normals (MetaVolume::mergeMV with addG, addH and blurnorms: gluvv's -addH and
 * -blurNormals; the data modes SMK_GDM_V1GH, _V2GH).  smk_merge_timestep with three flags: with nf = nelts - 1 - add_h, step
 * `step_out` becomes the step that smk_upload_timestep_device packs from what smk_merge_fields_h_device (ring SMK_U8) or
 * smk_merge_fields_h_f32_device (SMK_F32; SMK_U16 as in smk_merge_timestep: F = (float)v, G and H each through
 * smk_quantize_u16_device, H then stored as the pack's 8-bit field, the normals from the floats) make of the first nf stored
 * channels of `step_src`, bit for bit; the contract of the arithmetic stands at those entries below.  Channels: the nf fields,
 * G, and with add_h H.  With add_h = 0 and blur = 0 the stored bits are smk_merge_timestep's.
 * Two kernels on `stream`: pass 1 leaves {maximum magnitude, min H, max H} as ordered integers in three device words of the
 * OUTPUT slot, seeded on the stream; pass 2 writes the packed voxels, zeros in the pad column and row, and the brick summaries
 * follow.  No host wait, no allocation, no scratch arrays.  Slots, the in-place overwrite of a cached step_out, ordering and
 * refusals are smk_merge_timestep's.  Refused in addition, changing nothing: add_h or blur outside 0 / 1; nelts - 1 - add_h < 1;
 * add_h on a SMK_U16 ring with nelts != 3; a sharded context (the stencil reaches 2 voxels beyond region + halo and the scaling
 * needs the whole volume's three extremes: smk_step_extremes_h_device + smk_merge_timestep_h_shard below are the two-call
 * form, smk_block_extremes_h_device + smk_upload_timestep_fields_h_block_device the one from blocks). */
int smk_merge_timestep_h(smk_ctx *ctx, int step_src, int step_out, int add_h, int compat, int blur, void *stream);
/* The same from nf = nelts - 1 - add_h dense scalars in DEVICE memory, as smk_upload_timestep_fields_device takes them, with
 * that entry's additional refusals. */
int smk_upload_timestep_fields_h_device(smk_ctx *ctx, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                        int sx, int sy, int sz, int add_h, int compat, int blur, void *stream);
/* The two stencil producers on a SHARDED context (smk_set_shard), in two calls with one exchange of eight integers between
 * them; no voxel moves between ranks.  smk_derive_timestep and smk_merge_timestep above refuse a sharded context for two
 * reasons, and both go:
 *   - the extremes the result is scaled by are minima and maxima, which decompose exactly over the ranks' regions: every rank
 *     EXPORTS those of its region (smk_step_extremes_device), the host combines the ranks' words by elementwise integer
 *     maximum -- in-process ranks directly, a multi-process host with one integer MAX all-reduce of 8 words on its own
 *     transport --, and every rank runs the write pass with the combined words (smk_*_timestep_shard);
 *   - the stencil reaches r voxels (r = 2 for the derive, blurred or not; r = 1 for the merge; r = 2 for the merge with H,
 *     smk_merge_timestep_h_shard further below), and option "halo" lets a context keep that many and more.
 * THE WORDS.  Eight int32 in device memory.  A float x travels as its ordered int ord(x) = bits >= 0 ? bits : bits ^ 0x7fffffff
 * (ascending with x), and every MINIMUM as the bitwise complement of that, so that all eight words combine by maximum:
 *   SMK_EXTREMES_DERIVE  {~ord(min V), ord(max V), ~ord(min G), ord(max G), ~ord(min H), ord(max H), INT_MIN, INT_MIN}
 *                        over the region's interior voxels of the volume (V the source's channel 0, G and H the unscaled
 *                        gradient magnitude and second derivative; a NaN H is skipped), before the reference's +-1e8 seeds;
 *                        a region without an interior voxel exports the seeds {~ord(+inf), ord(-inf)} x 3
 *   SMK_EXTREMES_MERGE   {ord(max magnitude), INT_MIN x 7}: of the summed gradient over the region's interior voxels (a u8
 *                        ring: of all magnitudes; u16 and f32: of the finite ones); the seed is ord(0.0f) = 0
 * The maximum over the ranks' words equals, bit for bit, the words an unsharded context exports for the same step.
 * THE VALID BOX.  The result is exact on the SOURCE's valid box shrunk by r at every face of it that is not a face of the
 * volume (a face is the volume's when the source's valid box starts at voxel 0 or ends at the volume's last voxel; an
 * uploaded source is valid on the stored box cut at the volume, a block step on its C, which may end inside a stored box
 * that reaches the volume's face):
 * there every stored field and normal byte is what smk_derive_timestep / smk_merge_timestep store at that voxel on an
 * unsharded context -- the 1-voxel border (decided on the volume's coordinates) and the pad column and row included.  The
 * other stored voxels, the RIM, are written as zeros with the normal (128, 128, 128); zeros can only widen a brick's summary
 * range, so empty-space skipping stays conservative.  A source that has a rim itself (a second stencil) shrinks from its own
 * valid box.
 * THE VALID HALO.  Every cached step carries the number of halo voxels round the region that are exact: option "halo" after
 * an upload, the smaller of the sources' after a blend, the source's less r after these entries (on every rank of a
 * sharded series alike; unchanged on an unsharded context, which has no halo to lose).  smk_get_timestep_halo reads it.
 * A frame with perturbation or shadows on a shard compares its need with the SHOWN step's valid halo, and smk_probe_step
 * answers cells inside the step's valid box only.
 *
 * smk_step_extremes_device: pass 1 of the derive (`compat` as smk_derive_timestep's) or of the merge (`compat` ignored) over
 * this context's REGION of the cached step `step_src`, into the eight words at `d_words` (device memory, 4-byte aligned,
 * overwritten).  A reader of the step, ordered as smk_hist2d_step_device: enqueued on `stream` (NULL = the context's) behind
 * the step's writer; what overwrites the step later waits for it.  No host synchronisation, no allocation.  Refused, with the
 * reason: an unknown kind; d_words NULL or misaligned; no volume; the series' nelts (3 for the derive, >= 2 for the merge);
 * a volume thinner than 3 voxels; step_src not cached; a source whose valid halo is below r + 1 on a sharded context (the
 * message names both numbers). */
enum { SMK_EXTREMES_DERIVE = 0, SMK_EXTREMES_MERGE = 1, SMK_EXTREMES_MERGE_H = 2 /* a word layout, not a kind: smk_step_extremes_h_device */ };
int smk_step_extremes_device(smk_ctx *ctx, int kind, int step_src, int compat, void *d_words, void *stream);
/* The write pass alone: step `step_out` becomes the VGH step (derive) or the multi-field step (merge) of the cached step
 * `step_src`, scaled by the extremes in the eight words at `d_words` (device memory, read by the kernels on `stream`: the
 * caller orders its combine before them).  The words are NOT validated: words that are not the combined exports of this
 * step give a step scaled by whatever they say.  Producers like the one-call entries: the same slot rule (a cached step_out
 * is overwritten in place, otherwise a slot that is neither the source's nor the current step's), the same ordering on
 * `stream`, brick summaries for the result, no host synchronisation, no allocation.  They run on an unsharded context too:
 * there export + _shard stores the bits of smk_derive_timestep / smk_merge_timestep.  Refused, with the reason, changing
 * nothing: what smk_step_extremes_device refuses for the step; step_out < 0; step_out == step_src; no slot for the output
 * (the message names the slots needed).  The valid halo must be r + 1 because the result has to keep one halo voxel for a
 * frame's trilinear fetch. */
int smk_derive_timestep_shard(smk_ctx *ctx, int step_src, int step_out, int compat, int blur, const void *d_words, void *stream);
int smk_merge_timestep_shard(smk_ctx *ctx, int step_src, int step_out, const void *d_words, void *stream);
/* the valid halo of cached step `timestep` (an id, or SMK_STEP_CURRENT) */
int smk_get_timestep_halo(smk_ctx *ctx, int timestep, int *valid_halo);
/* ---- Blocks of a decomposed simulation: time steps from a rank's OWN dense block of the volume ("Blocks of a
 * decomposed simulation"; INTEGRATION.md 5, the in-situ recipe).  A simulation on P GPUs holds its sub-domain with ghost cells
 * on each GPU; the three device upload entries above have a BLOCK FORM that reads that array where it lies, wherever it lies
 * in the volume, so that no rank describes or assembles arrays it does not hold.
 * smk_block: `origin` is the global voxel of element [0][0][0] of the array handed over, `size` its voxels (x, y, z); the
 * pitches are the distances of two rows and of two slices in ELEMENTS (an element is one voxel of the array: a scalar, or the
 * nelts values of an interleaved voxel and the 3 bytes of its normal), 0 = contiguous: size[0] and size[0] * size[1].  The
 * block must lie inside the volume: a simulation whose array carries ghost cells outside the volume, or wider ghosts than it
 * wants to hand over, passes a VIEW -- the address of the view's first element, and the array's pitches.  Elements of the array
 * outside the view are never read.
 * THE VALID BOX OF A BLOCK, one rule for all three forms.  C = block ∩ stored box ∩ volume.  C must contain the context's
 * region [g0, g1), else the call is refused, naming the axis and both intervals.  The source's VALID HALO is the smallest
 * number of voxels C extends beyond the region, over the region's faces that are no faces of the volume, capped at option
 * "halo" (a side where C ends on the volume's own face gives all a halo can: no voxel lies beyond it); on an unsharded
 * context it is "halo", unchanged.  Stored voxels of the volume outside the result's valid box are
 * the RIM, zeros with the normal (128, 128, 128), as after smk_*_timestep_shard; the slot's valid halo and valid box are set
 * accordingly, and the frame path, smk_probe_step and every later producer respect them.
 * Refused by all block entries, changing nothing: a NULL block; a size <= 0; a pitch below the size (pitch_y < size[0],
 * pitch_z < pitch_y * size[1]); a block that leaves the volume; a block whose C does not contain the region. */
typedef struct {
  int origin[3];
  int size[3];
  long long pitch_y, pitch_z;
} smk_block;
/* The series' geometry WITHOUT data: leaves the context exactly as smk_upload_volume leaves it for a volume of zeros of
 * dims[3] voxels and extent[3] (volume space) with `normals` != 0 saying whether the series carries normals -- cached steps
 * dropped, the volume stored as the current step (id 0 on a new context, else the current id), packed zero voxels with the
 * normal (128, 128, 128), the pad, brick summaries, the shard's stored box (smk_set_shard and option "halo" before this
 * call), valid halo = "halo".  Refuses what smk_upload_volume refuses of such a volume, with the same words.  The only way
 * to give a sharded in-situ context its geometry; the block entries below need a volume, declared or uploaded.  Synchronous. */
int smk_declare_volume(smk_ctx *ctx, const int dims[3], const float extent[3], int nelts, smk_dtype dtype, smk_datamode dmode,
                       int normals);
/* The packed form: what smk_upload_timestep_device does with ONE brick at block->origin, pitched, without the requirement
 * that bricks tile the volume.  d_data is [z][y][x][nelts] of the series' dtype, d_grad_or_null [z][y][x][3] (present exactly
 * when the series has normals), both DEVICE memory read through the block's pitches.  The valid box is C, the valid halo the
 * source's; refused when that is below 1 on a sharded context (a frame's trilinear fetch needs one).  On an unsharded
 * context a block that is the whole volume stores smk_upload_timestep_device's bits.  Slot rule, ordering and refusals
 * otherwise as that entry's (no volume; timestep < 0; no slot); `stream` must also order the reads of the block. */
int smk_upload_timestep_block_device(smk_ctx *ctx, int timestep, const void *d_data, const unsigned char *d_grad_or_null,
                                     const smk_block *block, void *stream);
/* The stencil forms: smk_upload_timestep_scalar_device and smk_upload_timestep_fields_device from blocks, as two calls with
 * the eight-word exchange of smk_step_extremes_device between them.
 * Pass 1, smk_block_extremes_device: `kind` SMK_EXTREMES_DERIVE -- nf == 1, d_fields[0] the scalar, dtype any of SMK_U8,
 * SMK_U16, SMK_F32 whatever the ring's --, or SMK_EXTREMES_MERGE -- nf == nelts - 1 fields of the ring's dtype; d_fields is a
 * HOST array of nf device pointers read before the call returns, every array laid out by the one block.  The extremes of
 * the region's interior voxels go to the eight words at d_words, words and seeds as smk_step_extremes_device's: the maximum
 * over the ranks' words equals, bit for bit, what an unsharded context exports for the same scalar held as floats.
 * Pass 2, smk_upload_timestep_scalar_block_device / smk_upload_timestep_fields_block_device: the write pass with the
 * combined words, a producer into step `timestep` by smk_upload_timestep_device's slot rule.  The result's valid box is C
 * shrunk by the reach r (2 derive, 1 merge) at every face of C that is no face of the volume; its valid halo is the source's
 * less r on a sharded series.  A source valid halo below r + 1 on a sharded context is refused with both numbers.  Inside
 * the valid box every stored field and normal byte is what the unsharded entry stores at that voxel from the whole arrays:
 * the volume's 1-voxel border decided on global voxels, the pad column and row, u16's definition.
 * Refused, changing nothing: what the unsharded twins refuse (no volume; the series' nelts; a NULL or misaligned array; a
 * dtype that does not fit; nf; timestep < 0; no slot; d_words NULL or misaligned; an unknown kind) and what every block entry
 * refuses.  No host synchronisation, no allocation; `stream` (NULL = the context's) also orders the reads of the block. */
int smk_block_extremes_device(smk_ctx *ctx, int kind, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *block,
                              int compat, void *d_words, void *stream);
int smk_upload_timestep_scalar_block_device(smk_ctx *ctx, int timestep, const void *d_scalar, smk_dtype scalar_dtype,
                                            const smk_block *block, int compat, int blur, const void *d_words, void *stream);
int smk_upload_timestep_fields_block_device(smk_ctx *ctx, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                            const smk_block *block, const void *d_words, void *stream);
/* ---- Merged fields WITH H and blurred normals on a SHARDED context and from blocks: smk_merge_timestep_h and
 * smk_upload_timestep_fields_h_device as the same two calls with the same exchange of eight integers between them.  Entries
 * of their own because add_h decides which channels are fields (nf = nelts - 1 - add_h), which smk_step_extremes_device's
 * signature has no place for; SMK_EXTREMES_MERGE_H names their word layout and is no kind of that entry.
 * THE WORDS.  Eight int32, all combined by maximum as above:
 *   SMK_EXTREMES_MERGE_H  {ord(max magnitude), ~ord(min H), ord(max H), INT_MIN x 5}
 * over the REGION's interior voxels of the volume, the border decided on global voxels: the magnitude of the summed gradient
 * and, with add_h, its second derivative H, counted as pass 1 of smk_merge_timestep_h counts them (a u8 ring: every magnitude
 * and every H that is not NaN; u16 and f32: the finite ones).  The seeds are {0, ~ord(+inf), ord(-inf)}: with add_h == 0 words
 * 1 and 2 keep them, and a region without an interior voxel exports all three.  The write pass undoes the complement and then
 * applies the reference's +-1e8 seeds to min H and max H exactly as smk_merge_timestep_h does.  The maximum over the ranks'
 * words equals, bit for bit, the words an unsharded context exports for the same step.
 * THE REACH.  r = 2 for every combination of the flags: H reads the summed gradient of the six neighbours, a blurred normal that
 * of the 26, and each of those the fields one voxel further.  (A caller who wants reach 1 with no H and no blur has
 * smk_merge_timestep_shard.)  So a source valid halo below 3 on a sharded context is refused with both numbers; the result's
 * valid box is the source's (a block: C) shrunk by 2 at every face that is no face of the volume; its valid halo is the
 * source's less 2 on a sharded series, unchanged on an unsharded context; the rim is zeros with the normal (128, 128, 128);
 * the pad column and row are zeros.
 * THE CONTRACT.  Inside the valid box every stored field and normal byte is what smk_merge_timestep_h /
 * smk_upload_timestep_fields_h_device store at that voxel on an unsharded context from the whole volume.  On an unsharded
 * context, export followed by the write entry stores the one-call entry's bits.
 * smk_step_extremes_h_device: pass 1 over this context's region of the cached step `step_src` into the eight words at d_words
 * (device memory, 4-byte aligned, overwritten).  A reader of the step, ordered as smk_step_extremes_device.
 * smk_merge_timestep_h_shard: the write pass with the combined words; a producer like smk_merge_timestep_shard (slot rule,
 * in-place overwrite of a cached step_out, ordering on `stream`, brick summaries).  The words are not validated.
 * smk_block_extremes_h_device, smk_upload_timestep_fields_h_block_device: the same from nf = nelts - 1 - add_h dense fields of
 * the ring's dtype, every array laid out by the one block; F is taken as 0 outside C.  Reads no slot / a producer into step
 * `timestep`, as smk_block_extremes_device / smk_upload_timestep_fields_block_device.
 * No host synchronisation, no allocation in any of the four.  Refused, with the reason, changing nothing: add_h or blur outside
 * 0 / 1; nelts - 1 - add_h < 1; add_h on a SMK_U16 ring with nelts != 3; d_words NULL or misaligned; what
 * smk_step_extremes_device and smk_merge_timestep_shard (blocks: the block entries above) refuse, with reach 2; for blocks
 * d_fields NULL, a NULL or misaligned array, nf != nelts - 1 - add_h, a dtype that is not the ring's. */
int smk_step_extremes_h_device(smk_ctx *ctx, int step_src, int add_h, int compat, void *d_words, void *stream);
int smk_merge_timestep_h_shard(smk_ctx *ctx, int step_src, int step_out, int add_h, int compat, int blur, const void *d_words,
                               void *stream);
int smk_block_extremes_h_device(smk_ctx *ctx, const void *const *d_fields, int nf, smk_dtype dtype, const smk_block *block, int add_h,
                                int compat, void *d_words, void *stream);
int smk_upload_timestep_fields_h_block_device(smk_ctx *ctx, int timestep, const void *const *d_fields, int nf, smk_dtype field_dtype,
                                              const smk_block *block, int add_h, int compat, int blur, const void *d_words,
                                              void *stream);
/* ---- Halo refill: a cached step's stored halo copied, bit for bit, from the ranks that own those voxels ("Halo
 * refill"; INTEGRATION.md 5, the in-situ recipe).  The stencil producers above move no voxel between ranks and pay with the
 * valid halo; this is the one operation that moves voxels, and it is optional: a host that needs no more halo than survives
 * never calls it, and without a call every step, refusal and frame is what it is without these entries.  The regions
 * partition the volume and a sharded producer's result is exact on its region, so every voxel a rank lacks is held exactly by
 * exactly one other rank.  After the refill the step is the unsharded step's voxels on the whole stored box: valid box = the
 * stored box cut at the volume, valid halo = option "halo", no rim; frames, smk_probe_step and later producers treat it as
 * an uploaded step.  The shape is the light exchange's (smk_shadow_exports_device, _entries_device, _exchange_local).
 * `timestep` is a cached id or SMK_STEP_CURRENT.
 * GEOMETRY.  Rank r owns its region [g0_r, g1_r) (smk_set_shard's split).  Rank j stores S_j = [O_j, min(O_j + D_j, N)): the
 * region plus option "halo" voxels, cut at the volume, with the rule that evens the rows of 8-byte voxels in x and y -- one
 * more halo voxel where the volume has one, else the origin moved by one, else a pad column or row, which lies outside the
 * volume and is never touched.  Every rank computes every peer's box from the series' dims, dtype, nranks and the "halo" its
 * own stored box was made with: all ranks of a series must have the same.  Segment r->j (j != r) is the box region_r ∩ S_j; it
 * may be empty.  For every j, region_j and the segments i->j tile S_j exactly once.
 * SEGMENT FORMAT.  VB = 16 for SMK_F32 and 8 otherwise; NB = 4 where the slot has the separate normals buffer (4-channel f32
 * with normals), else 0.  A segment of n voxels is roundup16(n VB) bytes of packed voxels as stored, in z, y, x order with x
 * fastest, followed by roundup16(n NB) bytes of normal words in the same order.  The bytes a roundup adds are not written.
 * smk_step_halo_layout: send_bytes[j] = the length of segment r->j, recv_bytes[i] = that of segment i->r (index r: 0), and
 * their sums; any output may be NULL.  d_exports holds the segments to ranks 0..P-1 in rank order, back to back; d_entries
 * the segments from ranks 0..P-1 in rank order, back to back.  send_bytes of r to j equals recv_bytes of j from r, so a
 * multi-process host moves them with one all-to-all-v (grouped ncclSend / ncclRecv, or MPI_Alltoallv) whose counts and
 * displacements are these arrays and their prefix sums.  Needs a volume (uploaded or declared) and no step.
 * smk_step_halo_exports_device: a READER of the step, ordered as smk_hist2d_step_device: enqueued on `stream` (NULL = the
 * context's) behind the step's writer; what overwrites the step later waits for it.  Copies the voxels of this context's
 * region that lie in the peers' stored boxes into d_exports.
 * smk_step_halo_entries_device: an in-place WRITER of the cached step, which may be the current one.  On `stream` it comes
 * behind the frames and readers of the slot and behind its writer; the step keeps its id and its place in the ring.  It
 * scatters the segments into the stored halo (the region's own voxels are not written), makes the brick summaries again for
 * the whole stored box, drops the x-major copy, sets the valid box to S_j and the valid halo to "halo", records the slot's
 * readiness, and a current step is switched to as after an in-place upload.  The segments are NOT validated: entries that
 * are not the peers' exports of that step give a halo of whatever they hold.
 * smk_step_halo_exchange_local: both for the contexts of one process, ranks in order.  On one device every owner's slot is
 * copied straight into the receivers' slots -- exports read only regions and entries write only outside regions, so the
 * two never touch the same voxel and nothing is staged --, ordered per slot as a reader of the owner and a writer of the
 * receiver.  With a `stream` everything is enqueued on it and the host waits for nothing.  With NULL every receiver's copy
 * runs on its own context's stream and the host waits for all of them, before and after, as smk_shadow_exchange_local does.
 * Contexts on several devices take stream NULL and go through the two entries above with staging buffers the contexts keep and
 * peer copies between them.
 * One launch moves all of a rank's segments (at most nranks - 1 boxes, the table by value in the kernel's arguments); lanes
 * run along x, then y, then z of a box and move 16 bytes each.  No host synchronisation and no allocation in the two
 * _device entries.  On an unsharded context all byte counts are 0 and the entries return 0 and do nothing.  They are
 * idempotent: on a step whose halo is whole they store the same bits again.
 * Refused, with the reason, changing nothing: no volume; a step that is not cached; a NULL buffer where bytes are due; a
 * buffer below 16-byte alignment; in the local form: nranks outside 1..8 or different from the contexts' own, a context whose
 * rank is not its index, a context without a volume or without the step, contexts that differ from rank 0 in dims, dtype,
 * nelts, normals or "halo" (the message names the first rank that differs and the field), a `stream` with contexts on
 * several devices. */
int smk_step_halo_layout(smk_ctx *ctx, long long *send_bytes /*[nranks]*/, long long *recv_bytes /*[nranks]*/, long long *total_send,
                         long long *total_recv);
int smk_step_halo_exports_device(smk_ctx *ctx, int timestep, void *d_exports, void *stream);
int smk_step_halo_entries_device(smk_ctx *ctx, int timestep, const void *d_entries, void *stream);
int smk_step_halo_exchange_local(smk_ctx *const *all, int nranks, int timestep, void *stream);
/* introspection: the current step (-1: no volume), the cached ids oldest written first (min(cap, *n) of them; ids_out may
 * be NULL), their number */
int smk_get_timesteps(smk_ctx *ctx, int *current, int *ids_out, int cap, int *n);

/* Sort-last sharding (no reference equivalent: the reference draws bricks serially on one GPU,
 * NV20VolRen3D.cpp:190-231).  Must be called BEFORE smk_upload_volume: the context then keeps
 * only its convex sub-box (+1 voxel halo) of the volume.  nranks in {1,2,4,8}: split x, then y,
 * then z at the midpoint -- the MetaVolume::brick grid for a 2x2x2 bricking. */
int smk_set_shard(smk_ctx *ctx, int rank, int nranks);
/* front-to-back order of the ranks for the current camera (BSP rule per split axis) */
int smk_shard_order(smk_ctx *ctx, int *order_out /* nranks */);

/* replaces TLUT::loadTransferTableRGBA (TLUT.cpp:48-81): straight-colour float RGBA[size] as
 * held in TLUT::_rgba (already opacity-corrected by TLUT::scaleAlpha, which the caller keeps
 * doing exactly as VolumeRenderable::draw does, VolumeRenderable.cpp:50); premultiplied here. */
int smk_set_tlut1d(smk_ctx *ctx, const float *rgba, int size);
/* replaces NV20VolRen3D::loadDepTex x2 (NV20VolRen3D.cpp:1579-1622): deptex[sg][sv][RGBA8]
 * (gluvv.volren.deptex) and the optional third-axis table deptex2 (gluvv.volren.deptex2).  deptex2's alpha is multiplied
 * in only under the third-axis data modes (VGH, V1GH, V2G, V2GH, V3, V3G, V4; NV20VolRen3D.cpp:686-693) and only on a
 * volume of nelts >= 3: it is looked up at (third channel, fourth channel), the fourth being 0 when nelts is 3. */
int smk_set_tf2d(smk_ctx *ctx, const unsigned char *deptex, const unsigned char *deptex2_or_null,
                 int sv, int sg);
/* replaces TFWidgetRen::loadPtex for the dense table ptex[sh][sg][sv][RGBA8]
 * (TFWidgetRen.cpp:779-845) */
int smk_set_tf3d(smk_ctx *ctx, const unsigned char *ptex, int sv, int sg, int sh);

/* replaces the glGetDoublev(GL_MODELVIEW_MATRIX) + glFrustum state a renderer reads
 * (VolumeRenderable.cpp:40-49, gluvv.cpp:531-552): column-major modelview, frustum
 * {left,right,bottom,top} at clip[0] (near), window size (gluvv.win). */
int smk_set_camera(smk_ctx *ctx, const double modelview[16], const float frustum[4],
                   const float clip[2], int width, int height);
/* replaces R8kVolRen3D::loadCubeTex (R8kVolRen3D.cpp:2620-2679) / NV20VolRen3D::setupRegComb's
 * host half (NV20VolRen3D.cpp:637-668): gluvv.light.pos, gluvv.env.eye/at, gluvv.rinfo.xform,
 * gluvv.light.intens, gluvv.light.amb.  amb ("shadow strenght", gluvv.cpp:293) is consumed by frames with shadows in the NV20
 * look (smk_set_shadow, option "shadow_look" 1: the fraction of its colour a fully shadowed sample keeps; it must then be finite
 * and in [0, 1], or the render fails with the reason); every other frame stores it, unchecked and unused. */
int smk_set_shading(smk_ctx *ctx, smk_shade mode, const float light_pos[3], const float eye[3],
                    const float at[3], const float xform[16], float intens, float amb);
/* gluvv.volren.sampleRate / gamma / scaleAlphas (NV20VolRen3D.cpp:87-122).  steps > 0 fixes the
 * plane count instead (dis = view-depth extent / steps).  With scale_alphas the 2-D TF alpha is
 * corrected as copyScale does (NV20VolRen3D.cpp:1645-1660) with rate/gamma. */
int smk_set_sampling(smk_ctx *ctx, float sample_rate, int steps, float gamma, int scale_alphas);
/* replaces the orthogonal mode of the clip-plane widget (gluvv.clip.{on,ortho,oaxis,vpos},
 * gluvv.h:163-175; NV20VolRen3D::setupClips, NV20VolRen3D.cpp:251-327): the volume is drawn only
 * on one side of an axis-aligned plane through vpos (volume space, the units of fPos/fSize).
 * oaxis = VolRenMajorAxis: 1 X+ (x <= vpos.x stays), 2 X-, 3 Y+, 4 Y-, 5 Z+, 6 Z-.  on = 0: off. */
int smk_set_clip(smk_ctx *ctx, int on, int oaxis, const float vpos[3]);
/* replaces drawClip + renderSlice of the two live renderers (R8kVolRen3D.cpp:763-891, 893-921; NV20VolRen3D.cpp:329-502,
 * 506-528): in orthogonal mode they draw the slice of the data that lies on the clip plane, blended with gluvv.clip.alpha,
 * behind the volume when the plane faces away from the eye and on top of it when it faces the eye.  Drawn only while
 * smk_set_clip is on (its oaxis is used; free-mode planes draw no slice, R8kVolRen3D.cpp:800, NV20VolRen3D.cpp:363).
 *   corners = gluvv.clip.corners (CPWidgetRen::set_info, CPWidgetRen.cpp:215-296), volume space (the units of fPos / fSize);
 *   alpha   = gluvv.clip.alpha;
 *   dv      = dot(normalize(eye - clip.pos), normalize(clip.dir)), computed by the caller (R8kVolRen3D.cpp:273-281,
 *             NV20VolRen3D.cpp:124-131).
 * When: the slice is drawn BEFORE the volume when the case of oaxis holds for dv, AFTER it when it holds for -dv
 * (R8kVolRen3D.cpp:360-372, 400-424; NV20VolRen3D.cpp:144-148, 173-178): X+ dv < 0, X- dv > 0, Y+ dv > 0, Y- dv < 0, Z+ dv < 0,
 * Z- dv > 0 (R8kVolRen3D.cpp:826-879; the Y+ sign is the reference's), and -- except for X-, which the reference does not
 * test (:835) -- only if corner 0's clamped coordinate on that axis lies strictly inside (0, fSize).  dv == 0: neither.
 * Where: the corners are clamped to the volume box (:810-821), moved by +0.001 (X+, Y+, Z+) or -0.001 (X-, Y-, Z-) along
 * the axis (:823, 829-831 ...) and drawn as one GL_QUADS quad, triangles (0, 1, 2) and (0, 2, 3), texture coordinates =
 * the moved vertex / fSize (:906-913), GL_LINEAR, clamp to edge.
 * Colour: SMK_CLIP_LOOK_NV20 (final combiner, NV20VolRen3D.cpp:390, 426-431): src = (V a, V a, V a, a), V = the value channel,
 *   a = alpha.  SMK_CLIP_LOOK_R8K (createFragClip, R8kVolRen3D.cpp:3190-3250, textures per data mode :1926-2055): rgb = the
 *   data texel's first three channels in the third-axis data modes (four-byte texture); the texel with green replaced by
 *   its alpha otherwise -- (c0, c1, c0) for the two-byte modes V1G, V2, VGH_VG and (0, c0, 0) for the one-byte modes V1,
 *   VGH_V --, saturated; a = sat(alpha), src = (sat(rgb a), a) (:3223-3245).  u8 voxels decode / 255, f32 voxels are used
 *   as they are and saturated.
 * Order, onto the finished volume frame (GL_ONE, GL_ONE_MINUS_SRC_ALPHA, R8kVolRen3D.cpp:364, 404, 416): before pass
 * frame = volume + (1 - volume.a) src, after pass frame = src + (1 - a) volume.  Under SMK_BLEND_MAX the before pass is
 * max(volume, src) per component (the slice is in the framebuffer when GL_MAX starts, NV20VolRen3D.cpp:144-163).  With
 * shadows the before pass is skipped when the light runs along the view (axis[3] = vdl > 0, R8kVolRen3D.cpp:306-324, 360);
 * the after pass is always drawn; the slice never enters the light buffer.
 * Depth: the depth test is on, depth writes are off (R8kVolRen3D.cpp:365, 405, 417; NV20VolRen3D.cpp:433-434): under
 * smk_render_occluded a slice pixel exists only where its view depth is LESS than the scene depth; depth_out is not
 * changed by the slice (it reports volume samples).  On a shard every rank draws the part of the quad that lies in its own
 * region, before the exchange; the merged frame is the unsharded one where the pass is the one the geometry calls for
 * (before: the eye looks at the kept side of the plane; after: at the cut face), because everything beyond the slice, or
 * in front of it, is then clipped away in every rank; a pass that
 * contradicts the geometry is composed per rank all the same and merges to something else.  An after pass under
 * SMK_BLEND_MAX is refused on shards: a maximum cannot merge it.  on = 0, or smk_set_clip off: frames are bit-identical to those without this call
 * and nothing more is launched.  A bad look and non-finite corners, alpha or dv fail with the reason. */
typedef enum { SMK_CLIP_LOOK_NV20 = 0, SMK_CLIP_LOOK_R8K = 1 } smk_clip_look;
int smk_set_clip_slice(smk_ctx *ctx, int on, const float corners[4][3], float alpha, float dv, smk_clip_look look);
/* replaces the extents of VolumeRenderer::renderVolume(sampleRate, mv, xext, yext, zext) (VolumeRenderer.h:103-108,
 * VolumeRenderer.cpp:333-384, render3DVolumeEXTSV :428-505): only the axis-aligned sub-box lo..hi of the volume is drawn
 * (volume space, the units of fPos / fSize; clamped to the volume as :452-457 do; the reference's `x[1] -= origf[1]` slip,
 * :459, is not reproduced).  Planes stay the whole volume's.  on = 0: off.  A frame with shadows (smk_set_shadow) takes
 * the sub-box in both passes, as it takes an orthogonal clip plane's box. */
int smk_set_region(smk_ctx *ctx, int on, const float lo[3], const float hi[3]);
/* replaces the clip widget's free mode: glClipPlane(GL_CLIP_PLANE5, {0,0,-1,0}) specified under the
 * modelview wmv * T(clip.pos) * clip.xform (NV20VolRen3D.cpp:346-357; R8kVolRen3D.cpp:780-794).
 * plane_eye = the eye-space plane OpenGL stores for that call ({0,0,-1,0} times the inverse of that
 * matrix); a sample stays when plane_eye . (x_eye, 1) >= 0.  Both ray-marchers take it (the slice-ring kernel folds it
 * into each ray's plane interval: nothing per sample). */
int smk_set_clip_plane(smk_ctx *ctx, int on, const double plane_eye[4]);
/* replaces R8kVolRen3D_cpy::createNoiseTex + gluvv.pert (R8kVolRen3D_cpy.cpp:2392-2480,
 * 1590-1595): n^3 RGBA8 noise (GL_REPEAT), weights/scales of the two live octaves. noise NULL
 * or all weights 0 turns perturbation off.  Only the data fetch is displaced: p' = (t + sum_q w_q (noise(t s_q) - .5)) N - .5
 * for a sample at voxel coordinate p, t = (p + .5) / N; the sample exists, or not, by p itself (box, clip planes, scene
 * depth), and its first-hit depth is p's.  With shadows: see smk_set_shadow (option "shadow_perturb"). */
int smk_set_perturb(smk_ctx *ctx, const unsigned char *noise_rgba, int n, const float w[4],
                    const float s[4]);
/* replaces R8kVolRen3D's shadow mode (gluvv.light.shadow; gluvv.cpp:287-300 buffer size and qualities):
 * half-angle slicing.  The slice axis is the half-way vector of view and light direction
 * (R8kVolRen3D.cpp:296-326), every slice is drawn into the frame with its colour scaled by 1 - light
 * buffer (:1651-1740, shader :2928-2934) and then composited into the light buffer (:1760-1860, shader
 * :2991-3180) under the light's projection (LTWidgetRen::genXForm, LTWidgetRen.cpp:231-291).  Uses the
 * light position, eye, at and xform of smk_set_shading.  buffer_px = gluvv.light.buffsz[0], quality =
 * gluvv.light.gShadowQual or iShadowQual: the light buffer has ceil(quality * buffer_px)^2 texels.
 * Applies to 2-D / 3-D classification with no or R8k shading, with or without the clip-plane widget's planes
 * (smk_set_clip, smk_set_clip_plane: both passes leave out what lies beyond them, as the reference's clipped slice polygons
 * do), and with a sub-box (smk_set_region): to both passes the sub-box is what an orthogonal clip plane's box is -- the
 * eye box and the light box are intersected with it, its faces closed and 2^-10 voxels wide like a clip face, the slice set
 * stays the whole volume's.
 * Perturbation (smk_set_perturb) with shadows is what R8kVolRen3D_cpy draws -- volShadow binds the noise texture in both
 * passes (R8kVolRen3D_cpy.cpp:1566-1601), so the perturbed data drives the light buffer as well as the eye slices -- and
 * is OPT-IN: option "shadow_perturb" 1.  With the default 0 such a frame fails as it always has ("shadows cannot be combined
 * with perturbation or a sub-box"): an existing test pins that refusal, and hosts may rely on it; flipping the default,
 * together with that test, is a later one-line change.  With the option on: in both passes a sample exists, or not, by its
 * own position on the half-angle slice (the widened box, both clip planes, tau > 0, the scene depth in the eye pass);
 * nothing about membership, first-hit depth or the position the light buffer is looked up at depends on the noise; only
 * the data fetch (and, in the eye pass, the normal) is displaced, by the gather kernel's chain (smk_set_perturb above).  The
 * light-buffer recurrence is unchanged.  The eye pass of such a frame is the gather kernel's (auto mode lands there).
 * Still refused, with the reason: the 1-D table and NV20 combiners (those render under option "shadow_look" 1, below); perturbation or a sub-box with shadows on a shard
 * (smk_render and smk_shadow_exports_device) and under option shadow_fused; a forced slice-ring kernel ("kernel" 2) on a
 * perturbed frame; the column-stream kernel ("kernel" 3).  A shard (smk_set_shard) renders shadows once it has this frame's light entries (smk_shadow_exports_device,
 * smk_shadow_entries_device below; without them smk_render fails) and a halo of smk_get_shadow_margin's halo_needed.  The blend order follows the light (under when
 * the slices run away from the eye, over otherwise), smk_set_blend is not consulted.  depth_out works as without shadows:
 * the view depth of the nearest sample the eye pass composites along the pixel's half-angle ray (the shadow term scales
 * colour, never alpha, so it is the unshadowed frame's set of contributing samples, placed on the half-angle slices).
 * How it is rendered: a light-buffer texel depends on itself alone from slice to slice, so the light pass is
 * ONE march per texel that keeps every slice's buffer (nslices + 1 buffers in device memory), and the eye pass is an
 * ordinary frame of the ray-marchers over the half-angle slices that looks each sample's slice up -- two launches instead
 * of one per slice.  Option "shadow_march" 0 (or a history that does not fit a quarter of the free device memory) renders
 * a launch per slice as the reference draws them: the same samples, bit-identical light buffers.  The light buffers belong
 * to the context: its frames with shadows must be enqueued on ONE stream (they order themselves there).
 *
 * Option "shadow_look" chooses between the two shadow models of the reference.  0, the default, is all of the above: the R8k
 * look, coloured shadows (rgb *= 1 - light buffer rgb).  1 is the NV20 look: what the GeForce3 platform draws with shadows on,
 * through its fourth renderer NV20VolRen3D2 (gluvv.cpp:141-199 starts the renderers, :151-159 that one).  Its light pass is
 * the R8k one -- setupPBuff (NV20VolRen3D2.cpp:959-1091) blends the premultiplied slice (col a, a), a = a_VG a_H, into the
 * pbuffer with GL_ONE, GL_ONE_MINUS_SRC_ALPHA, the recurrence of R8kVolRen3D.cpp:3150-3165; volShadow (:1466-1585) copies the
 * pbuffer into the shadow texture before it draws slice k; axis and blend order (:174-200) are R8k's -- so light buffer and
 * history are bit-identical to look 0's for the same scene.  Its eye pass attenuates by the light buffer's OPACITY with an
 * ambient floor (setupRegComb, CONSTANT_COLOR1.a = 1 - gluvv.light.amb; unshaded :866-945, shaded :724-853): with La the
 * bilinear lookup of the light buffer's alpha where look 0 looks its colour up (zero border),
 *     f = 1 - sat(La) * (1 - amb),    amb of smk_set_shading, 1 - amb one fp32 subtraction,
 * SMK_SHADE_NONE gives rgb = sat(c f a) where look 0 has sat(c (1 - L.rgb) a), and SMK_SHADE_NV20_DIFF / _DSPEC give the
 * unshadowed NV20 sample's rgb times f (f = 1: that sample, bit for bit).  Alpha is a in either case: shadows are grey, a
 * fully shadowed sample keeps the fraction amb of its colour, and depth_out is look 0's.  Everything else is the frame
 * with shadows described above: clip planes, sub-box, first-hit depth, time steps, the clip-plane widget's slice, brick
 * flags, shards (the light exchange is look 0's).  Where this departs from NV20VolRen3D2 as coded -- its shaded combiners
 * lose the ambient floor and use another Phong -- DESIGN.md section 8 lists it.  Look 1 applies to 2-D / 3-D classification
 * with no or NV20 shading.  Refused under look 1, with the reason: R8k shading; the 1-D table; perturbation (with or
 * without "shadow_perturb"); option shadow_fused; the column-stream kernel; an amb that is not finite or outside [0, 1].
 * Look 0 refuses NV20 shading as before.  A frame with the host's scene depth (smk_render_occluded) under look 1 is the
 * gather kernel's: the slice-ring kernel has no such instance, auto mode lands on the gather kernel and a forced
 * "kernel" 2 fails with that reason.  A value other than 0 or 1 fails. */
int smk_set_shadow(smk_ctx *ctx, int on, int buffer_px, float quality);
/* replaces the glBlendFunc / glBlendEquationEXT state of the slice loop (VolumeRenderer.cpp:589-590,
 * NV20VolRen3D.cpp:158-163, 930; R8kVolRen3D.cpp:1436-1449).  Default: front to back.  The two
 * "over" orders are the same operator evaluated from opposite ends (equal up to fp32 rounding):
 * the gather kernel (option "kernel" 1) walks the planes of a back-to-front frame from the far one, as
 * the reference does; the slice-ring kernel composites such a frame front to back. */
int smk_set_blend(smk_ctx *ctx, smk_blend mode);

/* replaces gluvvPrimitive::draw() -> renderVolume (VolumeRenderer.cpp:280-328,
 * NV20VolRen3D.cpp:87-185): one frame.  rgba_out: [height][width][4] float, premultiplied,
 * row 0 = bottom (GL window order).  depth_out (may be NULL): view-space depth of the first
 * contributing sample, +inf where none. */
int smk_render(smk_ctx *ctx, float *rgba_out, float *depth_out);
/* same with DEVICE output pointers; asynchronous on `stream` (a hipStream_t, NULL = default).  (Option "kernel" 0: the
 * first nine frames of a configuration the context has not measured yet are trials of the two ray-marchers -- identical
 * frames -- and six of them wait for the frame before them on `stream`: a one-time stall per configuration.) */
int smk_render_device(smk_ctx *ctx, void *d_rgba, void *d_depth, void *stream);

/* ---- the host's opaque geometry in front of, behind and inside the volume.  The reference draws every slice with the
 * depth test on and depth writes off (R8kVolRen3D.cpp:380 "no depth wright, only depth test", :1447-1448;
 * NV20VolRen3D.cpp:932-933) under glDepthFunc(GL_LESS) (gluvv.cpp:559), into the frame gluvv's widgets and other primitives
 * were drawn into: opaque geometry hides the part of the volume behind it.  Here: a sample exists only if its view depth --
 * the value depth_out reports, tau * znear of smk_get_raycoef / smk_get_shadowcoef -- is LESS than the pixel's scene depth.
 * scene_depth: [height][width] floats of the whole window, row 0 = bottom (rgba_out's layout; the same full-window buffer
 * on a shard), of the kind
 *   SMK_SCENE_VIEW_DEPTH:   the view depth d itself (the units of smk_set_camera's clip);
 *   SMK_SCENE_WINDOW_DEPTH: what glReadPixels(GL_DEPTH_COMPONENT, GL_FLOAT) returns, z_w in [0, 1]; converted per pixel
 *                           to d = f n / (f - z_w (f - n)), (n, f) = smk_set_camera's clip, evaluated in DOUBLE precision
 *                           and rounded once to float (every kernel the same way).  z_w >= 1 (a cleared buffer) means no
 *                           occluder.
 * NaN means no occluder (+inf) in both kinds.  The test applies under every blend mode, depth_out, clip planes (both
 * forms), smk_set_region, perturbation, time steps, bricked uploads and shards.  With shadows only the eye pass is
 * occluded: the light buffer is the unoccluded frame's (the reference's light pbuffer holds the volume alone).  Option
 * "kernel" 3 (column-stream) refuses such frames; auto mode never takes it.  The clip-plane widget's slice
 * (smk_set_clip_slice) is tested the same way.  smk_render_slice is not affected.
 * smk_render_occluded copies scene_depth at the call; smk_render_occluded_device reads the DEVICE buffer d_scene_depth on
 * `stream` (the caller keeps it alive until the stream has passed the frame).  A NULL buffer makes them exactly smk_render /
 * smk_render_device.  A bad kind fails with the reason.  (INTEGRATION.md "Depth for the GL host".) */
typedef enum { SMK_SCENE_VIEW_DEPTH = 0, SMK_SCENE_WINDOW_DEPTH = 1 } smk_scene_depth_kind;
int smk_render_occluded(smk_ctx *ctx, const float *scene_depth, int kind, float *rgba_out, float *depth_out);
int smk_render_occluded_device(smk_ctx *ctx, const void *d_scene_depth, int kind, void *d_rgba, void *d_depth, void *stream);

/* ---- display-ready frames (DESIGN.md "Present").  The reference's frame IS the 8-bit GL framebuffer
 * its slices blend into, with the depth buffer beside it; smk_render hands the host 16 B per pixel of float RGBA in pageable
 * memory and leaves the depth conversion to it.  These entries deliver what the framebuffer takes: [height][width] RGBA8
 * (R in byte 0, row 0 = bottom) and, on request, [height][width] float32 window depths, in pinned host memory.
 *   Colour, q(x) = (uint8) floor(sat(x) * 255 + 0.5), NaN -> 0, fp32, one rounding per operation:
 *     bg NULL:  every channel c of the premultiplied frame, alpha included, becomes q(c);
 *     bg[3]:    an opaque background colour in [0, 1] drawn UNDER the frame -- the reference's white quad blended with
 *               GL_ONE_MINUS_DST_ALPHA, GL_ONE after the renderables (gluvv.cpp:606-623), for any colour --:
 *               rgb = q(C + (1 - A) * b), a = 255.
 *   Depth: the first-hit view depth d (depth_out of smk_render) becomes the window depth glReadPixels(GL_DEPTH_COMPONENT)
 *     would hold, z_w = f (d - n) / ((f - n) d) with (n, f) = smk_set_camera's clip, evaluated in DOUBLE, clamped to [0, 1]
 *     and rounded once to float: the inverse of SMK_SCENE_WINDOW_DEPTH's conversion.  d = +inf (nothing hit) or NaN gives
 *     exactly 1 (the cleared depth buffer), d <= n gives 0.  Needs f > n. */
/* replaces the host's own float -> 8-bit conversion and glDrawPixels(GL_FLOAT)'s, and the "convert on the
 * host" step of INTEGRATION.md 4: the conversion ALONE, asynchronous on `stream` (NULL: the context's stream), of any frame of
 * the context's window size in DEVICE memory -- of smk_render_device, merged by smk_composite_over[_depth]_device, an exchange
 * result on rank 0.  d_rgba: [h][w][4] floats, 16-byte aligned; d_rgba8: [h][w][4] bytes (16-byte aligned buffers are written
 * with 16-byte stores); d_depth_or_null / d_zwin_or_null: [h][w] floats each, both or neither. */
int smk_present_device(smk_ctx *ctx, const void *d_rgba, const void *d_depth_or_null, const float *bg_or_null, void *d_rgba8,
                       void *d_zwin_or_null, void *stream);
/* replaces gluvvPrimitive::draw() + the framebuffer the host then reads or blits (smk_render + the host's conversion): one
 * frame, synchronous -- the ray-march (smk_render_occluded's when scene_depth_or_null, HOST memory of kind scene_depth_kind,
 * is given), the conversion, the copy into pinned host buffers the context owns.  *rgba8 and *zwin (NULL when want_depth is 0;
 * either argument may be NULL) point INTO those buffers: see the slots below.  A frame the slice-ring kernel flags is handled
 * as smk_render handles it: in auto mode it is rendered again by the gather kernel before anything is returned, otherwise the
 * call fails. */
int smk_render_present(smk_ctx *ctx, const float *bg_or_null, const float *scene_depth_or_null, int scene_depth_kind,
                       int want_depth, const unsigned char **rgba8, const float **zwin);
/* the same frame in two calls (no reference equivalent: the reference renders synchronously).  _begin enqueues the ray-march and
 * the conversion on the context's stream and the copy to the host on a stream of its own behind them, and returns a ticket
 * (1, 2, ...) at once: frame k's copy runs beside frame k + 1's ray-march.  _end waits for that ticket's copy and returns the
 * pointers; a flagged frame is treated as by smk_render_present (the second rendering is synchronous and uses the context's
 * state at _end).  There are TWO slots, taken in turn; each owns everything its frame needs while in flight -- RGBA8 and
 * window-depth device buffers, their pinned copies, its copy of scene_depth (taken at _begin) -- so:
 *   - a slot's pointers stay valid and its bytes unchanged until the SECOND _begin after its own (smk_render_present is a
 *     _begin + _end and counts as one);
 *   - a third _begin while two tickets are outstanding is refused;
 *   - smk_set_camera with another window size is refused while a ticket is outstanding;
 *   - an unknown or already ended ticket is refused;
 * each with the reason in smk_last_error.  The float frame is the context's own, written and read in stream order.  Pinned
 * memory is allocated at a slot's first frame, again when the window's pixel count changes, and released by smk_destroy.
 * smk_last_frame_info reports the frame _end returned; smk_get_stat "present_ms" / "present_bytes" its conversion and copy. */
int smk_render_present_begin(smk_ctx *ctx, const float *bg_or_null, const float *scene_depth_or_null, int scene_depth_kind,
                             int want_depth, long long *ticket);
int smk_render_present_end(smk_ctx *ctx, long long ticket, const unsigned char **rgba8, const float **zwin);

/* replaces VolumeRenderer::renderSlice(quad, alpha) (VolumeRenderer.h:114, VolumeRenderer.cpp:748-807): ONE quad (model
 * space, the units of fPos / fSize; drawn as glBegin(GL_QUADS) with the vertices in the order 1, 0, 2, 3) textured with the
 * scalar volume -- GL_INTENSITY8, GL_LINEAR, no colour table (:768), texture coordinates = vertex / fSize -- modulated by
 * glColor4f(1, 1, 1, alpha) and blended GL_ONE, GL_ONE_MINUS_SRC_ALPHA into the frame:
 *   src = (I, I, I, I * alpha), frame = src + (1 - src.a) * frame,   I = the first data channel in [0, 1].
 * Uses the camera of smk_set_camera.  rgba_inout: [height][width][4] float, read and written.  (Not the clip-plane widget's
 * slice, smk_set_clip_slice: that one is part of the frame -- ordered against the volume, depth-tested, drawn on shards --
 * and takes its colour from the renderers' data texel, not from GL_INTENSITY8.) */
int smk_render_slice(smk_ctx *ctx, const float quad[4][3], float alpha, float *rgba_inout);
int smk_render_slice_device(smk_ctx *ctx, const float quad[4][3], float alpha, void *d_rgba_inout, void *stream);

/* Frames in flight (no reference equivalent: the reference renders synchronously).  smk_render_device
 * only enqueues; the slice-ring kernel reports a protocol time-out or a window outside its host bound
 * through a per-frame status word.  smk_last_frame_id: id of the frame the last smk_render_device call
 * enqueued (1, 2, ...).  smk_frame_failed: call after synchronising with that frame's stream; 1 = the
 * frame was flagged and must be rendered again (option "kernel" = 1 renders it on the gather kernel),
 * 0 = valid, -1 = unknown (never enqueued, or older than the last 8 frames).  Asking consumes the answer.
 * The host may enqueue frame i + 1 before it asks about frame i (the pipelined protocol of the sort-last
 * merge): a render call only looks at the status slot it takes over -- a flagged frame nobody asked
 * about while it could be asked about makes the render call 8 frames later fail.  The synchronous
 * smk_render re-renders a flagged frame itself.  Status words carry their frame's id, so a word that
 * arrives after its slot was handed on is not blamed on the younger frame.  All of it is counted
 * (smk_get_stat "slab_failures" / "slab_retries") so a test or a benchmark can require zero. */
long long smk_last_frame_id(smk_ctx *ctx);
int smk_frame_failed(smk_ctx *ctx, long long frame_id);

/* sort-last merge: out = layer[order[0]] over layer[order[1]] over ...; layers are
 * premultiplied RGBA tiles of npix pixels, DEVICE pointers, layer l at layers + l*npix*4 floats. */
int smk_composite_over_device(smk_ctx *ctx, const void *d_layers, int nlayers, const int *order,
                              int npix, void *d_out, void *stream);
/* the same merge with first-hit depth (no reference equivalent: the north star's final reduce of per-brick RGBA + depth
 * segments).  d_depths: [nlayers][npix] floats, layer l's depth at d_depths + l*npix, each the depth_out of
 * smk_render_device on that shard (+inf where it has no sample).  d_out gets the RGBA of smk_composite_over_device, bit
 * for bit; d_depth_out[p] = the minimum of the layers' depths at p (+inf where none is finite).  Every blend mode merges
 * depth by minimum: a context reports its NEAREST contributing sample (front to back the first composited, back to front
 * the last, GL_MAX the first), every sample belongs to one shard and all shards place samples on one plane set, so the
 * minimum over the shards is the unsharded frame's depth, bit for bit.  One pass over the pixels. */
int smk_composite_over_depth_device(smk_ctx *ctx, const void *d_layers, const void *d_depths, int nlayers,
                                    const int *order, int npix, void *d_out, void *d_depth_out, void *stream);

/* ---- the sort-last merge in C (no reference equivalent): one object per rank = per
 * context / GPU.  Direct send of the 1/P image tiles (grouped ncclSend/ncclRecv over xGMI), ordered
 * over of the P layers in smk_shard_order's order, finished tiles gathered on rank 0.
 *   RCCL transport (id != NULL): one process per GPU.  Rank 0 makes the 128-byte communicator id
 *     (smk_exchange_unique_id = ncclGetUniqueId) and hands it to the other ranks by whatever channel
 *     the host has; smk_exchange_create is then collective (ncclCommInitRank).  librccl is opened at
 *     run time.
 *   in-process transport (id == NULL): the ranks are contexts of ONE process (a C++ host that owns
 *     several GPUs): create all, smk_exchange_connect_local, then smk_exchange_frame_local per frame.
 * A rank renders frame i into smk_exchange_partial(x, i & 1) -- [npix][4] floats, device -- after
 * smk_exchange_acquire(x, i & 1, render_stream), and marks it with smk_exchange_rendered(x, i & 1,
 * render_stream); smk_exchange_frame enqueues that frame's merge on the exchange's own stream behind
 * that mark and returns at once, so frame i's merge overlaps frame i+1's ray-marching (which may
 * already be enqueued: a host checks smk_frame_failed for frame i in between).  d_frame ([npix][4], rank 0 only) receives the merged frame;
 * smk_exchange_wait makes a stream wait for everything enqueued so far.  A NULL stream means the
 * context's own stream, as in smk_render_device.  The context must have been sharded with the same
 * rank / nranks (smk_set_shard). */
typedef struct smk_exchange smk_exchange;
#define SMK_EXCHANGE_ID_BYTES 128
int smk_exchange_unique_id(unsigned char id[SMK_EXCHANGE_ID_BYTES]);
smk_exchange *smk_exchange_create(smk_ctx *ctx, int rank, int nranks, const unsigned char *id, int npix, int *err);
int smk_exchange_connect_local(smk_exchange *const *all, int nranks);
void smk_exchange_destroy(smk_exchange *x);
const char *smk_exchange_last_error(smk_exchange *x); /* x may be NULL: last smk_exchange_create failure */
void *smk_exchange_partial(smk_exchange *x, int slot);
int smk_exchange_acquire(smk_exchange *x, int slot, void *render_stream);
int smk_exchange_rendered(smk_exchange *x, int slot, void *render_stream);
/* The shards' visibility order of the frame in `slot` is taken from the context's camera at the first
 * smk_exchange_rendered after smk_exchange_acquire -- i.e. under the pose the frame was rendered with, not the one current
 * when the merge is enqueued; a host that knows better (a frame re-rendered later, a replayed sequence) sets it itself:
 * order[nranks], front to back (smk_shard_order's convention). */
int smk_exchange_set_order(smk_exchange *x, int slot, const int *order);
int smk_exchange_frame(smk_exchange *x, int slot, void *d_frame);
int smk_exchange_frame_local(smk_exchange *const *all, int nranks, int slot, void *d_frame);
int smk_exchange_wait(smk_exchange *x, void *stream);
/* First-hit depth through the exchange (no reference equivalent: the north star's RGBA + depth reduce).
 * smk_exchange_partial_depth: the [npix] float plane a rank renders slot `slot`'s depth into (smk_render_device's
 * d_depth, beside smk_exchange_partial(x, slot)).  The first call allocates a depth plane beside each RGBA buffer of both
 * slots (rendered layer, received tiles, finished tile; +inf in the padding) and returns NULL only if that fails; from then
 * on the exchange carries depth: the depth pieces travel with the RGBA pieces (inside the same ncclGroupStart/End; the
 * in-process transport with the same copies and events), the merge takes the minimum of the depths in the same pass as
 * the ordered over (smk_composite_over_depth_device's rule, every blend mode), and frames go through the _depth entries
 * below -- smk_exchange_frame[_local] refuse a depth-carrying exchange, the _depth entries one that never enabled depth,
 * and in-process ranks must all carry depth or none.  d_depth ([npix] floats) is rank 0's only, like d_frame.  The merged
 * depth equals the unsharded frame's bit for bit.  An exchange that never asks for depth allocates and moves exactly
 * what it did before: 16 B per pixel; with depth 20. */
void *smk_exchange_partial_depth(smk_exchange *x, int slot);
int smk_exchange_frame_depth(smk_exchange *x, int slot, void *d_frame, void *d_depth);
int smk_exchange_frame_local_depth(smk_exchange *const *all, int nranks, int slot, void *d_frame, void *d_depth);

/* data prep on the GPU (genVGH/main.cpp:56-182, VectorMath.h:874-899,
 * 1133-1148, 1217-1281).  All pointers are DEVICE pointers.
 *   scalar  [z][y][x] u8, f32 or u16 -> vgh_u8 [z][y][x][3] (quantised as makeVGH) and/or
 *                                       vgh_f32 [z][y][x][3] in [0,1] (unquantised variant)
 *   vgh_u8                           -> normals [z][y][x][3] (derivative3DVGH+[blurV3D]+scalebiasN)
 * A SMK_U16 scalar gives, in both outputs, the bits of the SMK_F32 call on the same values converted with (float)v. */
int smk_make_vgh_device(smk_ctx *ctx, const void *d_scalar, smk_dtype dtype, int sx, int sy,
                        int sz, int compat, void *d_vgh_u8_or_null, void *d_vgh_f32_or_null);
int smk_normals_vgh_device(smk_ctx *ctx, const void *d_vgh_u8, int nelts, int sx, int sy, int sz,
                           int blur, void *d_normals);
/* replaces MetaVolume::mergeMV with addG (MetaVolume.cpp:1109-1268; AGradArb VectorMath.h:945-1004,
 * GMag :1010-1030, scalebiasN :1133-1148): nf (1..3) co-registered scalar fields, interleaved
 * [z][y][x][nf] u8 -> d_out [z][y][x][nf+1] with the magnitude of the SUMMED per-field gradient as
 * last element, and optionally the normal bytes [z][y][x][3] of that gradient.  Device pointers;
 * bytes identical to the reference arithmetic. */
int smk_merge_fields_device(smk_ctx *ctx, const void *d_fields_u8, int nf, int sx, int sy, int sz,
                            void *d_out, void *d_normals_or_null);
/* replaces MetaVolume::hist2D (MetaVolume.cpp:1650-1688; caller TFWidgetRen::loadHist,
 * TFWidgetRen1.cpp:660-700): the log-scaled joint histogram of the (value, gradient) bytes,
 * hist[g*256 + v], 65536 bytes in HOST memory; bit-identical to the reference's, including its
 * float bins that stop counting at 2^24.  nelts < 2 is refused as there.  _device: the volume
 * [z][y][x][nelts] is already in device memory. */
int smk_hist2d(smk_ctx *ctx, const smk_volume_desc *bricks, int n_bricks, int nelts, unsigned char *hist);
int smk_hist2d_device(smk_ctx *ctx, const void *d_vol_u8, int nelts, int sx, int sy, int sz, unsigned char *hist);
/* The three entries above for FLOAT volumes [z][y][x][channels] f32: these extend the reference's byte
 * arithmetic with the loads widened and the final quantisation dropped.  All pointers are DEVICE
 * pointers, the work runs on the context's stream and each call synchronises before it returns.  Every step is plain
 * fp32, one rounding per operation in the order written, so a float32 restatement gives the same bits.
 *
 * smk_normals_f32_device extends MetaVolume::normalsVGH = derivative3DVGH + optional blurV3D + scalebiasN
 * (VectorMath.h:874-899, 1217-1281, 1133-1148): the gradient of channel 0, g[e] = d[o + stride_e] - d[o - stride_e] (one
 * fp32 subtraction, 0 on the 1-voxel border); blur != 0 applies smk_normals_vgh_device's weights, 27-term order,
 * interior-only sources and divisor; the bytes are those of smk_normals_vgh_device's scalebiasN step (nrm_store in
 * smk_prep.hip), +1 -> 255 clamp included.  If a component of the gradient handed to that step is not finite, the voxel
 * gets the zero vector's bytes (128, 128, 128).  d_normals is [z][y][x][3] u8, what smk_upload_volume_device /
 * smk_upload_timestep_device take as grad.  The reference has no float pipeline. */
int smk_normals_f32_device(smk_ctx *ctx, const void *d_f32, int nelts, int sx, int sy, int sz, int blur, void *d_normals);
/* extends MetaVolume::mergeMV with addG (MetaVolume.cpp:1109-1268; AGradArb VectorMath.h:945-1030): nf (1..3) fields
 * interleaved [z][y][x][nf] f32, dims >= 3, -> d_out [z][y][x][nf+1] f32.  out[..., 0:nf] are the input floats bit for
 * bit; out[..., nf] = mag / maxm (one fp32 division), mag = sqrtf(g0*g0 + g1*g1 + g2*g2) of the SUMMED gradient (fields
 * ascending, one add per field and axis, 0 on the border), maxm the maximum of mag over the voxels whose mag is finite.
 * A voxel whose mag is not finite gets G = 0, and every voxel does when maxm is 0.  The optional normals [z][y][x][3] u8
 * come from the summed gradient by smk_normals_f32_device's rule.  The reference has no float pipeline: its GMag
 * quantises to a byte, (uchar)(mag / max * 255), which is what is dropped here. */
int smk_merge_fields_f32_device(smk_ctx *ctx, const void *d_fields_f32, int nf, int sx, int sy, int sz, void *d_out_f32,
                                void *d_normals_or_null);
/* MetaVolume::mergeMV with addG, addH and blurnorms (MetaVolume.cpp:1109-1268; gluvv.cpp's -addH and -blurNormals): the two
 * merge entries above with H and blurred normals.  d_fields is [z][y][x][nf], d_out [z][y][x][nf + 1 + add_h], bytes (_h_device)
 * or floats (_h_f32_device); nf is 1..3, and 1..2 with add_h; dims >= 3; add_h and blur are 0 or 1; synchronous, as their twins.
 * With add_h = 0 and blur = 0 they store the bits of smk_merge_fields_device / smk_merge_fields_f32_device.  The contract, with
 * S the summed gradient exactly as there (fields ascending, one fp32 subtraction and one add per field and axis, 0 on the
 * volume's 1-voxel border):
 *   G.  Unchanged: (uchar)(|S| / max * 255.0), or |S| / maxm in floats.  G and H come from the UNBLURRED S, as mergeMV
 *       computes them before blurV3D (MetaVolume.cpp:1217-1256).
 *   H.  GMagHess (VectorMath.h:1032-1113) is a copy of makeVGH's second-derivative block (genVGH/main.cpp:103-175) in which
 *       three reads name the output array `hess`, never yet written, where the copy's source names the computed value
 *       (:1086-1087, :1099): as coded it reads uninitialised memory and has no defined result.  Built here: those three reads
 *       take `tmph`, i.e. makeVGH's lines.  An interior voxel has hs = the second derivative along the gradient from S and S at
 *       its six neighbours (smk_make_vgh_device's expression; compat != 0 keeps the `tg[1] +` typo of :1078, 0 uses h[4]).  A
 *       border voxel has hs = 0 -- NOT makeVGH's zeroed border: 0 takes the `else` branch of the scaling and quantises to 85
 *       (floats: (float)(85.0 / 255.0)) wherever max H is not 0.  hmin and hmax run over the interior voxels from the seeds
 *       +1e8 and -1e8; a NaN (zero gradient) never wins.  The byte / float is makeVGH's scaling of hs with those extremes
 *       (255 / 3 and 255 / 3 * 2 are the integers 85 and 170); the byte of a NaN is 0.
 *       Floats: hmin and hmax run over FINITE hs only, and a voxel whose hs is not finite gets H = 0 (the rule maxm follows).
 *   Blurred normals.  blur != 0: the normal's gradient is blurV3D of S -- smk_normals_vgh_device's weights, 27-term
 *       source-raster order, interior-only sources and divisor -- then the twins' byte rule.  blur == 0: S itself.
 *   Fields.  Copied as by the twins, border included.
 * The float entry refuses pointers below float alignment. */
int smk_merge_fields_h_device(smk_ctx *ctx, const void *d_fields_u8, int nf, int sx, int sy, int sz, int add_h, int compat,
                              int blur, void *d_out, void *d_normals_or_null);
int smk_merge_fields_h_f32_device(smk_ctx *ctx, const void *d_fields_f32, int nf, int sx, int sy, int sz, int add_h, int compat,
                                  int blur, void *d_out_f32, void *d_normals_or_null);
/* extends MetaVolume::hist2D (MetaVolume.cpp:1650-1688): a channel's bin is b(v) with t = v * 255.0f (one fp32
 * multiply): NaN or t < 0 -> 0, t >= 255 -> 255, otherwise (int)t.  Counts go to hist[b(c1) * 256 + b(c0)] and are
 * finished as smk_hist2d_device's (log scale, float bins that stop at 2^24); hist is 65536 bytes in HOST memory and
 * nelts < 2 is refused as there.  d_vol_f32 needs float alignment only.  The reference has no float pipeline. */
int smk_hist2d_f32_device(smk_ctx *ctx, const void *d_vol_f32, int nelts, int sx, int sy, int sz, unsigned char *hist);
/* ---- the histogram and the probe of a RESIDENT time step (DESIGN.md 3b "Histogram and probe of a step").  The entries above
 * take the raw [z][y][x][nelts] array; a step that came from a device buffer (smk_upload_timestep_device), a blended step
 * (smk_blend_timesteps), a shard's region and SMK_U16 voxels have none, so these read what the context owns: the packed
 * voxels of a ring slot.  `timestep` is the id of a cached step, as smk_select_timestep takes it, or SMK_STEP_CURRENT; any
 * other value fails with "not cached", as there. */
#define SMK_STEP_CURRENT (-1)
/* replaces MetaVolume::hist2D's counting loop (MetaVolume.cpp:1650-1688) for that step: 65536 uint32 counts into DEVICE
 * memory, counts[b1 * 256 + b0], overwritten, not accumulated.  Every voxel of this context's region [g0, g1) of the step is
 * counted exactly once -- never a halo voxel, never the extra voxel or the pad column that evens out 8-byte rows; on an
 * unsharded context the region is the whole volume, and shard regions partition it (smk_set_shard), so the sum of the ranks'
 * counts is the unsharded context's.  Bins, b0 from channel 0 and b1 from channel 1:
 *   SMK_U8   the byte itself: smk_hist2d_device's counts on the uploaded array;
 *   SMK_F32  smk_hist2d_f32_device's rule: t = v * 255.0f (one fp32 multiply), NaN or t < 0 -> 0, t >= 255 -> 255, else (int)t;
 *   SMK_U16  v / 257 in integer arithmetic = floor(255 v / 65535) exactly, 65535 -> 255; no float is involved.
 * Refused, with the reason: no volume; nelts < 2 ("needs value and gradient channels"); a step that is not cached; a NULL
 * d_counts.  Asynchronous, as smk_blend_timesteps: everything is enqueued on `stream` (NULL = the context's) behind the
 * step's upload or blend, and a later upload or blend INTO that slot waits for this read.  No host synchronisation. */
int smk_hist2d_step_device(smk_ctx *ctx, int timestep, void *d_counts, void *stream);
/* replaces MetaVolume::hist2D (MetaVolume.cpp:1650-1688; caller TFWidgetRen::loadHist, TFWidgetRen1.cpp:660-700) for that
 * step: the same work on the context's stream, synchronous; the 65536 counts and / or smk_hist2d's log-scaled 256 x 256 bytes
 * into HOST memory.  At least one of the two outputs must be given. */
int smk_hist2d_step(smk_ctx *ctx, int timestep, unsigned *counts_or_null, unsigned char *hist_or_null);
/* replaces the scaling half of MetaVolume::hist2D (MetaVolume.cpp:1672-1688), which every histogram entry above ends with:
 * 65536 counts -> 65536 bytes, min(count, 2^24) as float (the reference's float bins stop there), log, scaled by the maximum.
 * Host memory only, no context: a sharded host sums its ranks' counts and finishes once.  NULL arguments fail. */
int smk_hist2d_finish(const unsigned *counts, unsigned char *hist);
/* replaces the data fetch of TFWidgetRen::drawProbe (TFWidgetRen1.cpp:309-595; host/TransferFunctions.cpp probe_sample) for
 * that step: the 2 x 2 x 2 corner voxels of n cells (1..65536), synchronous.  cells[n][3]: whole-volume voxel coordinates
 * (x, y, z) of each cell's low corner; corner i * 4 + j * 2 + k is the voxel (x + k, y + j, z + i): probe_sample's order.
 *   raw_out[n][8][4]  the STORED values as floats, nothing rescaled: SMK_U8 the bytes 0..255; SMK_U16 channels 0 and 1 as
 *                     0..65535, channel 2 as its stored 8-bit value 0..255, channel 3 zero; SMK_F32 the floats bit for bit;
 *                     a channel the volume lacks is 0;
 *   nrm_out[n][8][3]  (may be NULL) the normal bytes, (128, 128, 128) when the volume has none;
 *   ok_out[n]         1 when all eight corners lie inside the volume AND inside the box this context stores (region + halo;
 *                     the pad column is outside the volume), else 0 and that cell's outputs are zeros: a sharded host asks
 *                     every rank and takes whichever answers.
 * Refused, with the reason: no volume, a step that is not cached, a missing pointer, n out of range. */
int smk_probe_step(smk_ctx *ctx, int timestep, const int *cells, int n, float *raw_out, unsigned char *nrm_out_or_null,
                   int *ok_out);
/* ---- a resident time step read back: raw voxels and normals from the packed voxels of a ring slot, the inverse of the
 * upload's pack (DESIGN.md 3b "Reading a step back").  These stand in for MetaVolume::writeAll / Volume::writeVol
 * (MetaVolume.cpp:99-126, 963-1000), which write the host's currentData / currentGrad: a step uploaded from device memory,
 * a blended step and a shard's region have neither, so what is read is what the context owns -- the slot's packed voxels,
 * and the separate normals of four-channel f32; never the x-major copy.  `timestep` as for smk_hist2d_step_device. */
/* the box smk_download_timestep* returns: this context's region [g0, g1) -- origin = g0, size = g1 - g0 in voxels (x, y, z)
 * -- and the type of what comes back.  Unsharded: origin 0, size = the volume.  Any out pointer may be NULL.  Stands in for
 * the sizes writeAll puts into the .trex (MetaVolume.cpp:963-1000).  Refused without a volume. */
int smk_get_timestep_box(smk_ctx *ctx, int origin[3], int size[3], int *nelts, smk_dtype *dtype, int *has_normals);
/* stands in for Volume::writeVol's source (MetaVolume.cpp:99-126, 963-1000) for that step, into DEVICE memory of this
 * context's GPU.  The box is the region, exactly smk_hist2d_step_device's set of voxels: never a halo voxel, never the extra
 * voxel or the pad column that evens out 8-byte rows; shard regions partition the volume, so the ranks' boxes placed at
 * their origins assemble it with nothing written twice.
 *   d_data  [sz][sy][sx][nelts] of the step's dtype -- unsigned char, float, or uint16_t in host byte order;
 *   d_grad  (may be NULL) [sz][sy][sx][3] unsigned char;
 * both dense, no padding; d_data needs its element's alignment only (anything less is refused), d_grad none.  EXACTLY
 * sx * sy * sz * nelts * sizeof(element) and sx * sy * sz * 3 bytes are written: no byte before or after either buffer is
 * touched, whatever its alignment.
 * Values are the stored fields, nothing rescaled:
 *   SMK_U8   the channel bytes;
 *   SMK_F32  the floats bit for bit -- NaN payloads, infinities and -0 included;
 *   SMK_U16  channels 0 and 1 as their 16 bits; channel 2 as 257 * q, q the stored 8-bit field.  That is the limit of the
 *            TYPE (the packed voxel keeps 8 bits of a third channel, smk.h SMK_U16), not of the download; and since
 *            q8(257 q) = (65535 q + 32767) / 65535 = q, uploading the result stores the same voxel again;
 *   normals  the three normal bytes; a step without normals gives (128, 128, 128), as smk_probe_step does.
 * So download(upload(x)) == x bit for bit for u8, f32 and the first two u16 channels, and upload(download(step)) into a
 * fresh context packs identical voxels: frames and step histograms are bit-identical.
 * Asynchronous, with smk_hist2d_step_device's ordering: everything is enqueued on `stream` (NULL = the context's) behind the
 * step's upload or blend, and the slot's reader event is recorded behind it, so a later upload or blend INTO that slot
 * waits for this read.  It neither holds up nor is held up by the frames that render the step.  No host synchronisation.
 * Refused, with the reason: no volume; a step that is not cached; a NULL d_data. */
int smk_download_timestep_device(smk_ctx *ctx, int timestep, void *d_data, void *d_grad_or_null, void *stream);
/* stands in for MetaVolume::writeAll + Volume::writeVol (MetaVolume.cpp:99-126, 963-1000) for that step: the same work on
 * the context's stream into staging device buffers of the box's size, copied out to HOST memory; synchronous.  `data` needs
 * no alignment.  Refused as above, and -- with the bytes named -- when the staging buffers do not fit in free device memory. */
int smk_download_timestep(smk_ctx *ctx, int timestep, void *data, unsigned char *grad_or_null);
/* the bridge from the float prep entries (smk_make_vgh_device's vgh_f32, smk_merge_fields_f32_device) to SMK_U16 voxels (no
 * reference equivalent: the reference quantises to bytes): n_values floats -> n_values uint16_t, DEVICE pointers, on the
 * context's stream, synchronous like its siblings.  Per value t = v * 65535.0f (one fp32 multiply): NaN or t < 0 -> 0,
 * t >= 65535 -> 65535, otherwise (uint16_t)(int)(t + 0.5f) -- one fp32 add, then truncation.  Plain fp32 in that order, so a
 * float32 restatement gives the same bits. */
int smk_quantize_u16_device(smk_ctx *ctx, const void *d_f32, long long n_values, void *d_u16);
/* synthetic scalar test volumes generated on the GPU (u8, [z][y][x]):
 *   kind 1 = the reference's own generator: `genvol -spheres 4 -p 10 -pscale .7 -pwrap 3 3 3 -pabs -blur
 *            -bw 1 1 1 .7` with srand(seed) (genvol/main.cpp:153-165, 212-256, 334-430; perlin.c; script
 *            genvol/scripts/make64.bat:1) -- bytes identical to a CPU run of that tool on glibc
 *   kind 0 = smooth noisy concentric shells (analytic, no staircase; round-1 bench input) */
int smk_synth_volume_device(smk_ctx *ctx, int kind, unsigned seed, int sx, int sy, int sz,
                            void *d_scalar_u8);

/* introspection used by tests and bench (no reference equivalent) */
typedef struct {
  float pxs, pxl, pys, pyl;
  float Ac[3], Ax[3], Ay[3], Bc[3], Bx[3], By[3];
  int nplanes;
  float tau0, dtau, zmin, zmax, dis;
} smk_raycoef;
int smk_get_raycoef(smk_ctx *ctx, smk_raycoef *out);
/* sample placement of a frame with shadows: slice k = 1..nslices in the light's order.  A light-buffer texel's sample is
 * fma(w, G, Lc) with G_a = fma(a, Gx_a, fma(b, Gy_a, Gc_a)), (a, b) = fma(texel + .5, las, lal),
 * w = fma(k, ldnum, lnum0) / fma(a, nGx, fma(b, nGy, nGc)).  An eye ray's planes are counted FROM THE EYE, m = k - 1 when the
 * slices run away from the viewer (front_to_back), nslices - k otherwise: with D_a = fma(px, Dx_a, fma(py, Dy_a, Dc_a)),
 * nD = fma(px, nDx, fma(py, nDy, nDc)), numA = plane 0's numerator (fma(1, dnum, num0) or fma(nslices, dnum, num0)) and
 * dB = +-dnum:  tauA = numA / nD, dtau = dB / nD, A_a = fma(tauA, D_a, Ec_a), B_a = dtau * D_a, sample = fma(m, B, A), which
 * exists where fma(m, dtau, tauA) is positive and finite and lies within 2^-10 voxels of the volume's box.  X/Y/Wm map a
 * voxel coordinate to light space, its light-buffer position is fma(x'/w, lscale, lbias) (DESIGN.md "Shadows") */
typedef struct {
  float pxs, pxl, pys, pyl;
  float Ec[3], Dc[3], Dx[3], Dy[3];
  float nDc, nDx, nDy, num0, dnum;
  float las, lal;
  float Lc[3], Gc[3], Gx[3], Gy[3];
  float nGc, nGx, nGy, lnum0, ldnum;
  float Xm[4], Ym[4], Wm[4];
  float lscale, lbias;
  int nslices, LB, front_to_back;
} smk_shadowcoef;
int smk_get_shadowcoef(smk_ctx *ctx, smk_shadowcoef *out);
/* the light buffer as the last frame with shadows left it: [LB][LB][4] floats to HOST memory (synchronises) */
int smk_get_light_buffer(smk_ctx *ctx, float *rgba_out, int *lb_out);
/* the light buffer after slices 1..k (k = 0..nslices; 0 = cleared) of the last frame with shadows rendered with the two
 * marches: [LB][LB][4] floats to HOST memory (synchronises).  On a shard only the texels whose slice-k sample lies within
 * the margin of the shard's region hold the unsharded frame's values (they are all its eye pass looks up). */
int smk_get_light_history(smk_ctx *ctx, int k, float *rgba_out);

/* Shadows on shards ("Shadows on shards").  The reference draws the bricks of a shadowed volume one after
 * another against one light buffer (R8kVolRen3D.cpp:582-679, volShadow :1651-1868); here every rank marches its own light
 * samples.  A light-buffer texel's ray crosses the shards' boxes in the light's BSP order, so the buffer rank j reads is
 * E_j over H_j: H_j = j's own march over the samples within its margin m of its region, E_j = the other ranks' samples
 * before the ray reaches that, which they send.  Per frame, after the camera, light and tables are set on every rank:
 *   1. smk_shadow_exports_device on every rank r: X_{r->j} for every rank j, [nranks][LB][LB][4] floats (slot r zero),
 *      enqueued on `stream` (NULL: the context's stream);
 *   2. every rank j receives slot j of every rank's exports, in rank order, [nranks][LB][LB][4] floats, and hands them to
 *      smk_shadow_entries_device (copied on `stream`, consumed by the next smk_render[_device] -- which fails without);
 *   3. smk_render[_device] on every rank, merged with smk_composite_over_device in smk_shard_order's order.
 * smk_shadow_exchange_local runs steps 1-2 for contexts of one process (device-to-device copies, peer copies between
 * devices; it synchronises every rank's stream).  The halo (option "halo", before upload) must be at least
 * smk_get_shadow_margin's halo_needed = m + 1.  Frames stay within a few ulp of the unsharded frame (the over of the light
 * buffer is associated differently).  Not provided: a transport of the light exchange over RCCL (smk_exchange_* with an id:
 * a host moves the exports itself between steps 1 and 2), bench.py legs, and shards with option shadow_march 0 or
 * shadow_fused (the per-slice and cooperative paths stay single-GPU: smk_render fails). */
int smk_shadow_exports_device(smk_ctx *ctx, void *d_exports, void *stream);
int smk_shadow_entries_device(smk_ctx *ctx, const void *d_entries, void *stream);
int smk_shadow_exchange_local(smk_ctx *const *all, int nranks);
/* the ranks in the light's BSP order, nearest the light first (smk_shard_order's rule from the light rays' apex) */
int smk_shard_light_order(smk_ctx *ctx, int *order_out /* nranks */);
/* margin m (voxels) of this shard's frame with shadows and the halo it needs (m + 1); per frame: it follows the light */
int smk_get_shadow_margin(smk_ctx *ctx, int *m, int *halo_needed);
/* Empty-space skipping (option "bricks", no reference counterpart: the reference draws every slice and lets the blend
 * unit discard what the table made transparent, VolumeRenderer.cpp:507-741).  The flags the NEXT frame would use, for
 * checkers: one byte per brick of 8x8x8 cells of this context's stored box, x fastest, 1 = some sample whose cell lies
 * in the brick may be visible under the current table.  nb_out[3] receives the brick counts; flags_out may be NULL to
 * ask for the counts alone; *in_use_out (may be NULL) tells whether frames use them (not for a 1-D colour table, with
 * the option off, or once > 90 % of the bricks turned out flagged).  Needs volume, table and camera; synchronises. */
int smk_get_brick_flags(smk_ctx *ctx, unsigned char *flags_out, int *nb_out, int *in_use_out);
/* options (all optional; defaults in brackets):
 *   "kernel"   [0] 0 auto: both ray-marchers produce bit-identical frames, the first frames of a new
 *              configuration time one and the other and the faster is kept; 1 gather kernel (every
 *              mode); 2 slice-ring kernel (fails where it does not apply, with the reason); 3 column-stream
 *              kernel (smk_cols.hip: the volume re-laid out in columns with their halo, streamed sequentially,
 *              a ray's per-column partial composites merged in order -- the same samples, the blend
 *              re-associated: <= 2e-5 from the other two; fails where it does not apply)
 *   "slab_split" [0] depth segments of the slice-ring kernel: 0 = tiles measured long are rendered by several
 *              workgroups where the longest tile stands above the mean load of a workgroup slot (sharded
 *              contexts), the partial frames merged in order (<= 2e-5 from the unsplit frame); 1 = never
 *              (bit-identical to the gather kernel everywhere); 2..8 = every tile in that many.  Frames with a
 *              depth output are never cut (the merge pass knows colours only)
 *   "tf_raw"   [0] 1: the 2-D table handed to smk_set_tf2d is already opacity-corrected (copyScale off)
 *   "halo"     [1] voxels of halo kept around a shard's region (before smk_upload_volume)
 *   "bricks"   [1] empty-space skipping: 8x8x8-cell bricks in which no sample can be visible under the current
 *              table are neither streamed nor sampled (the skipped samples are exactly transparent: frames are
 *              bit-identical with 0 and 1); 0 = every sample is fetched and classified
 *   "shadow_march" [1] frames with shadows as two marches (light-buffer texels, then eye pixels on the ray-marchers);
 *              0 = a launch per slice
 *   "shadow_perturb" [0] 1: a perturbed frame with shadows renders (smk_set_shadow); 0: it is refused, as before
 *   "shadow_look" [0] the shadow model of frames with shadows (smk_set_shadow): 0 the R8k look (1 - light-buffer colour),
 *              1 the NV20 look of NV20VolRen3D2 (light-buffer opacity, ambient floor amb of smk_set_shading)
 *   developer knobs: "tile" (slice-ring workgroup shape id), "slab_T" (band wait + 1), "slab_fly"
 *   (slices a loader keeps in flight), "slab_ns" (cap on the ring's slots), "lockstep" (bit 0 gather lockstep; bits 1..6 slice-ring
 *   diagnostics, see tools/kbench.py), "wave_w"/"blk_w" (gather tile shape), "inject_slab_status"
 *   (test hook: the next slice-ring frame reports this status word) */
int smk_set_option(smk_ctx *ctx, const char *key, int value);
/* samples of the current frame set-up that lie inside the volume (region and clip planes counted in): the renderers'
 * membership test for every plane of every ray, nothing fetched (with shadows on: the eye pass's half-angle slices).  SURVEY 8(d)'s "in-volume sample count", to be read
 * beside the nominal width x height x planes.  Synchronises. */
int smk_count_samples(smk_ctx *ctx, double *in_volume);
/* last frame: which kernel ran (1 gather, 2 slice-ring, 3 the per-slice shadow passes of option shadow_march 0, 4 column-
 * stream; a frame with shadows reports the kernel of its eye pass, its time covers the light march too), its HIP-event time
 * in ms, algorithmic bytes */
int smk_last_frame_info(smk_ctx *ctx, int *kernel, float *ms, double *alg_bytes);
/* HIP-event timing of the render kernel on its launch stream: reset, render N frames, read the
 * average (ms) over the last min(N,64) frames.  smk_timing_read synchronises the device. */
int smk_timing_reset(smk_ctx *ctx);
int smk_timing_read(smk_ctx *ctx, float *avg_ms, int *nframes);
/* named counters of the last frame (developer statistics, no reference counterpart):
 * "slab_iters", "slab_active_lanes", "slab_inside_lanes" (lanes that interpolate a sample: not skipped as part of an
 * empty layer), "slab_hit_lanes", "slab_iters_with_maybe" (turns in which a lane passes the table's occupancy bit),
 * "slab_visible_kcyc", "slab_texel_wait_kcyc" (cycles of those turns' visible path, and of them waiting for the table
 * texels) (collected when option
 * lockstep has bit 16 set), "slab_status" (these synchronise the device); "light_samples" (the light-march samples of
 * the current frame with shadows this context owns -- all of them on the whole volume; synchronises); "slab_failures",
 * "slab_retries" (host-side counters, no synchronisation); "clip_slice_pass" (which pass of smk_set_clip_slice the last
 * frame's rule chose: 0 none, 1 before the volume, 2 after it; no synchronisation); "present_ms" (the HIP-event time of the
 * conversion kernel of the last frame smk_render_present[_end] returned, or of the last smk_present_device -- then it waits for
 * that kernel), "present_bytes" (the bytes the last frame smk_render_present[_end] returned copied to the host: 4 per pixel,
 * 8 with depth); "tblend_count" (blends smk_blend_timesteps has enqueued on this context; no synchronisation).
 * "slab_plan_<field>": the launch plan of the latest slice-ring frame, as the host derived it from camera, volume size and
 * voxel type (host memory, no synchronisation; every field reads 0 unless smk_last_frame_info reports kernel 2).  Fields:
 *   tw th nw nl        the workgroup's pixel tile, its consumer and its loader waves
 *   wu wv wp           the window: 16-byte units loaded per row, rows, LDS row pitch in units
 *   per rpg            DMA wave-instructions and rows per row group: wp / gcd(64, wp), 64 / gcd(64, wp)
 *   groups chunks      row groups per slice = ceil(wv / rpg); DMA wave-instructions per slice = groups * per
 *   mych               the most DMA wave-instructions ONE loader issues per slice
 *   nslots maxfly      the ring's slots; slices a loader keeps in flight
 *   wstep pmask        slices a wave waits for beyond its band; consumers publish progress when (turn & pmask) == 0
 *   mask_need use_occ use_ah fast_tf   per-slice extents; occupancy bitmap / third-axis alpha table in LDS; alpha-first path
 *   bricks             1 when the brick flags are in use (empty layers), else 0
 *   perm dir           principal axis (0: S = z, 1: S = y, 2: S = x on the x-major copy); marching direction +1 / -1
 *   lds_bytes          the workgroup's LDS allocation
 *   slices_max         slices the longest tile's loaders have to stream (its positions + 1), from the host's window scan
 * The column-stream kernel (option "kernel" 3) of the latest frame: "cols_builds" (column layouts built so far),
 * "cols_config" (cw | ch << 8 | nslots << 16 | shape << 24), "cols_jobs", "cols_stream_bytes" (host memory); "cols_job_ms_max",
 * "cols_job_ms_sum", "cols_setup_ms_sum", "cols_rays" (over the jobs' workgroups; synchronise); with option "cols_counts" on
 * "cols_samples", "cols_visible", "cols_slices", "cols_segments", "cols_iters", "cols_active_lanes", "cols_switch_iters",
 * "cols_switch_lanes" (synchronise).
 * "cols_plan_<field>": the launch plan of the latest column-stream frame (host memory, no synchronisation; every field reads
 * 0 unless smk_last_frame_info reports kernel 4).  Fields:
 *   cw ch ncu ncv      cells per column along U and V; columns (the pad voxel of a box of 8-byte voxels is no cell)
 *   slice_bytes        a column's slice image: (cw + 1)(ch + 1) voxels, rounded up to 16 bytes
 *   n_ch last_units    DMA wave-instructions per slice = ceil(slice_bytes / 1024); lanes (16-byte units) of the last one, 1..64
 *   nslots maxfly      the ring's slots (option "cols_ns" caps them); slices one loader keeps in flight ("cols_fly")
 *   wstep              slices a wave waits for beyond the two it reads ("cols_wstep" - 1), at most nslots - 2
 *   take_min take_wait a wave takes new rays when this many lanes are free, or after this many turns ("cols_take_min",
 *                      "cols_take_wait" - 1)
 *   cl nck             slice positions per chunk ("cols_chunk" caps them, 4..256); chunks
 *   nkeys mask_words   segment keys = ncu + ncv + nck - 2; 64-bit mask words per pixel, at most 8
 *   shape              workgroup shape: 0 = 15 consumer waves + 1 loader, 1 = 14 + 2 ("cols_shape" - 1)
 *   perm dir           principal axis (0: S = z, 1: S = y, 2: S = x); marching direction +1 / -1 */
int smk_get_stat(smk_ctx *ctx, const char *name, double *value);
/* workgroup timeline of the last slice-ring frame (developer tool):
 * records of 8 x uint32 {start, end (100 MHz ticks), HW_ID, XCC_ID | tile<<8 | slices<<20, loader 0's
 * issue / vmcnt-wait / ring-blocked time in units of 64 cycles, sum of the consumer waves' iterations};
 * with option lockstep bit 32 set the records come from the diagnostic kernel instances, one per workgroup;
 * without it from the product kernel itself, one per tile (the first four words; a tile cut in depth segments
 * leaves its record empty).
 * *nrecords = records available; copies min(cap_records, *nrecords) when out != NULL. */
int smk_get_trace(smk_ctx *ctx, unsigned *out, int cap_records, int *nrecords);
/* effective 2-D TF after opacity correction (sg*sv*4 bytes) and the rate it was corrected with.  This is a HOST
 * recomputation: the alpha map of the current rate applied to the host copy of the raw table -- not a read-back of
 * what the device kernel wrote into the table version the frames fetch from.  The device table, its occupancy bitmap
 * and the brick flags built on it are checked through frames and flags in tests/test_gpu_tf_correction.py. */
int smk_get_tf2d_effective(smk_ctx *ctx, unsigned char *out, float *rate_out);

#ifdef __cplusplus
}
#endif
#endif
