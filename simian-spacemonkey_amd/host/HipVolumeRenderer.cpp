// HipVolumeRenderer.cpp -- see the header.  Every GL call of the reference path is replaced by
// one smk_* call; everything else (who owns what, when tables are re-sent, error style) follows
// the reference files cited inline.
#include "HipVolumeRenderer.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <climits>
#include <cstdio>
#include <iostream>
#include <string>

#include "VolumeFiles.h"  // smkfiles::write_trex / write_nrrd (saveTimeStep)

static void build_modelview(double mv[16]);  // LookAt * T(trans) * R(xform) * T(-size/2)
static void build_world_modelview(double mv[16]);
static void mul(double o[16], const double a[16], const double b[16]);
static void translate(double m[16], double x, double y, double z);

HipVolumeRenderer::HipVolumeRenderer(MetaVolume *vm, int, int device)
    : ctx(nullptr), m_vol(vm), tlut(nullptr), pmode(HipPresentFloat), pdepth(0), pticket(0), pW(0), pH(0), fb8(nullptr), zb(nullptr), failed(0), m_bb(0), m_bbb(0), m_u16(0) {
  int err = 0;
  ctx = smk_create(device, &err);
  if (!ctx) {
    std::cerr << "ERROR: HipVolumeRenderer: " << smk_last_error(nullptr) << std::endl;
    failed = 1;
  }
  // gluvv.pert.on and gluvv.light.shadow together are what the perturbing renderer this class mirrors draws
  // (R8kVolRen3D_cpy::volShadow, :1566-1601): the C ABI's opt-in for that combination (smk.h, smk_set_shadow)
  if (ctx) smk_set_option(ctx, "shadow_perturb", 1);
  // the GeForce3 platform draws gluvv.light.shadow with NV20VolRen3D2 (gluvv.cpp:151-159): the light buffer's opacity with
  // the ambient floor gluvv.light.amb -- the C ABI's NV20 look (smk.h, smk_set_shadow); every other platform keeps the R8k look
  if (ctx && gluvv.plat == GPNV20) smk_set_option(ctx, "shadow_look", 1);
}

HipVolumeRenderer::~HipVolumeRenderer() {
  if (tlut) delete tlut;  // VolumeRenderer.h:89
  smk_destroy(ctx);
}

// the bricks of a MetaVolume as the renderer reads them (currentData / currentGrad: the time step swapped in)
static std::vector<smk_volume_desc> brick_descs(Volume *v, int n) {
  std::vector<smk_volume_desc> d(n);
  for (int i = 0; i < n; ++i) {
    d[i].xiSize = v[i].xiSize; d[i].yiSize = v[i].yiSize; d[i].ziSize = v[i].ziSize;
    d[i].xfSize = v[i].xfSize; d[i].yfSize = v[i].yfSize; d[i].zfSize = v[i].zfSize;
    d[i].xiPos = v[i].xiPos; d[i].yiPos = v[i].yiPos; d[i].ziPos = v[i].ziPos;
    d[i].xfPos = v[i].xfPos; d[i].yfPos = v[i].yfPos; d[i].zfPos = v[i].zfPos;
    d[i].data = v[i].currentData;
    d[i].grad = v[i].currentGrad;
  }
  return d;
}

int HipVolumeRenderer::upload(Volume *v, int n) {
  if (!ctx) return 1;
  std::vector<smk_volume_desc> d = brick_descs(v, n);
  if (smk_upload_volume(ctx, d.data(), n, m_vol->nelts, m_u16 ? SMK_U16 : SMK_U8, (smk_datamode)gluvv.dmode)) {
    std::cerr << "ERROR: HipVolumeRenderer::createVolume: " << smk_last_error(ctx) << std::endl;
    failed = 1;
    return 1;
  }
  return 0;
}

int HipVolumeRenderer::hist2D(unsigned char *hist) {
  if (!ctx || !m_vol || !m_vol->volumes) return 0;
  if (m_u16) {  // (the histogram's bins are the reference's bytes: uint16_t voxels have none)
    std::cerr << "MetaVolume::hist2D, not implemented for 16-bit voxels" << std::endl;
    return 0;
  }
  std::vector<smk_volume_desc> d((size_t)m_vol->numSubVols);
  for (int i = 0; i < m_vol->numSubVols; ++i) {
    const Volume &v = m_vol->volumes[i];
    memset(&d[(size_t)i], 0, sizeof(smk_volume_desc));
    d[(size_t)i].xiSize = v.xiSize; d[(size_t)i].yiSize = v.yiSize; d[(size_t)i].ziSize = v.ziSize;
    d[(size_t)i].data = v.currentData;
  }
  if (smk_hist2d(ctx, d.data(), m_vol->numSubVols, m_vol->nelts, hist)) {
    std::cerr << "MetaVolume::hist2D, " << smk_last_error(ctx) << std::endl;
    return 0;  // the reference's "not implemented" return
  }
  return 1;
}

int HipVolumeRenderer::hist2DStep(unsigned char *hist) {
  if (!ctx || !hist) return 0;
  if (smk_hist2d_step(ctx, SMK_STEP_CURRENT, nullptr, hist)) {
    std::cerr << "MetaVolume::hist2D, " << smk_last_error(ctx) << std::endl;
    return 0;
  }
  return 1;
}

int HipVolumeRenderer::probeStep(const float vpos[3], smktf::ProbeSample *out) {
  if (!ctx || !m_vol || !vpos || !out) return 0;
  const int sx = m_vol->xiSize, sy = m_vol->yiSize, sz = m_vol->ziSize;
  float raw[8][4];
  memset(raw, 0, sizeof raw);
  smktf::probe_sample_raw(raw, 0, sx, sy, sz, gluvv.dmode, vpos, out);  // the cell and its test
  if (!out->inside) return 1;
  int ok = 0;
  if (smk_probe_step(ctx, SMK_STEP_CURRENT, out->cell, 1, &raw[0][0], nullptr, &ok)) {
    std::cerr << "ERROR: HipVolumeRenderer::probeStep: " << smk_last_error(ctx) << std::endl;
    return 0;
  }
  if (!ok) {
    std::cerr << "HipVolumeRenderer::probeStep: cell " << out->cell[0] << " " << out->cell[1] << " " << out->cell[2]
              << " is not held by this context" << std::endl;
    out->inside = false;
    return 0;
  }
  smktf::probe_sample_raw(raw, m_u16 ? SMK_U16 : SMK_U8, sx, sy, sz, gluvv.dmode, vpos, out);
  return 1;
}

int HipVolumeRenderer::downloadStep(std::vector<unsigned char> *data, std::vector<unsigned char> *grad, int origin[3], int size[3]) {
  if (!ctx || !data) return 0;
  int o[3], s[3], nelts = 0;
  smk_dtype dt = SMK_U8;
  if (smk_get_timestep_box(ctx, o, s, &nelts, &dt, nullptr)) {
    std::cerr << "ERROR: HipVolumeRenderer::downloadStep: " << smk_last_error(ctx) << std::endl;
    return 0;
  }
  const size_t nvox = (size_t)s[0] * (size_t)s[1] * (size_t)s[2];
  data->resize(nvox * (size_t)nelts * (dt == SMK_U8 ? 1 : dt == SMK_U16 ? 2 : 4));
  if (grad) grad->resize(nvox * 3);
  if (smk_download_timestep(ctx, SMK_STEP_CURRENT, data->data(), grad ? grad->data() : nullptr)) {
    std::cerr << "ERROR: HipVolumeRenderer::downloadStep: " << smk_last_error(ctx) << std::endl;
    return 0;
  }
  for (int a = 0; a < 3; ++a) {
    if (origin) origin[a] = o[a];
    if (size) size[a] = s[a];
  }
  return 1;
}

int HipVolumeRenderer::createVolume(int type, Volume *v) {
  if (type != VolRen3DExt) {  // VolumeRenderer.cpp:103-112: the other modes "not implemented"
    std::cerr << "texture mapping method is not implemented" << std::endl;
    return 1;
  }
  return upload(v, 1);
}

int HipVolumeRenderer::createVolume(int type, Volume *v, int nVols) {
  if (type != VolRen3DExt) {
    std::cerr << "texture mapping method is not implemented" << std::endl;
    return 1;
  }
  return upload(v, nVols);
}

int HipVolumeRenderer::createTLUT() {
  tlut = new HipTLUT;
  return 1;
}

// TLUT::scaleAlpha (TLUT.cpp:138-154) up to, not including, its loadTransferTableRGBA() call
int HipTLUT::scaleAlphaNoUpload(float sampleRate) {
  if (lastSampleRate == sampleRate) return 0;
  float alphaScale = lastSampleRate / sampleRate;
  lastSampleRate = sampleRate;
  for (int i = 0; i < _size; ++i) _rgba[i * _numElts + 3] = 1 - pow((1 - _rgba[i * _numElts + 3]), alphaScale);
  return 1;
}

void HipVolumeRenderer::loadTransferTableRGBA() {
  if (!ctx || !tlut) return;
  if (smk_set_tlut1d(ctx, tlut->GetRGBA(0), tlut->GetSize())) {
    std::cerr << "ERROR: HipVolumeRenderer::loadTransferTableRGBA: " << smk_last_error(ctx) << std::endl;
    failed = 1;
  }
}

// the frame in flight, waited for: its pinned buffers become framebuffer8() / depthbuffer()
int HipVolumeRenderer::endTicket() {
  if (!pticket) return 0;
  const long long t = pticket;
  pticket = 0;
  const unsigned char *p8 = nullptr;
  const float *pz = nullptr;
  if (smk_render_present_end(ctx, t, &p8, &pz)) return 1;
  fb8 = p8;
  zb = pz;
  return 0;
}

void HipVolumeRenderer::present(HipPresentMode mode, int want_depth) {
  if (!ok()) return;
  if (endTicket()) {  // (a frame enqueued under the old mode is not lost)
    std::cerr << "ERROR: HipVolumeRenderer::present: " << smk_last_error(ctx) << std::endl;
    failed = 1;
  }
  pmode = mode;
  pdepth = want_depth;
}

void HipVolumeRenderer::flush() {
  if (!ok()) return;
  if (endTicket()) {
    std::cerr << "ERROR: HipVolumeRenderer::flush: " << smk_last_error(ctx) << std::endl;
    failed = 1;
  }
}

// gluvv.env.bgColor as display() reads it (gluvv.cpp:606-623): 0 draws a white quad UNDER the finished frame
// (GL_ONE_MINUS_DST_ALPHA, GL_ONE), anything else leaves the cleared black
void HipVolumeRenderer::renderPresent() {
  static const float white[3] = {1.0f, 1.0f, 1.0f};
  const float *bg = gluvv.env.bgColor == 0 ? white : nullptr;
  const size_t npix = (size_t)gluvv.win.width * (size_t)gluvv.win.height;
  if (pmode == HipPresentSync) {
    if (endTicket() || smk_render_present(ctx, bg, nullptr, 0, pdepth, &fb8, &zb)) failed = 1;
    return;
  }
  // pipelined: this frame is enqueued BEFORE the one in flight is waited for, so that its ray-march runs beside that copy
  const long long before = pticket;
  long long t = 0;
  if (smk_render_present_begin(ctx, bg, nullptr, 0, pdepth, &t)) {
    failed = 1;
    return;
  }
  pticket = before;
  if (before) {
    if (endTicket()) failed = 1;
  } else {  // the first frame: nothing has arrived yet
    blank8.assign(npix * 4, 0);
    blankz.assign(npix, 1.0f);
    fb8 = blank8.data();
    zb = pdepth ? blankz.data() : nullptr;
  }
  pticket = t;
}

void HipVolumeRenderer::renderVolume(float sampleRate, double mv[16]) {
  if (!ok()) return;
  const int W = (int)gluvv.win.width, H = (int)gluvv.win.height;
  if (pmode != HipPresentFloat) {
    // (a frame in flight owns buffers of the window it was enqueued with: it is handed over before the window changes)
    if (pticket && (pW != W || pH != H) && endTicket()) failed = 1;
    pW = W;
    pH = H;
    int rc = failed || smk_set_camera(ctx, mv, gluvv.env.frustum, gluvv.env.clip, W, H);
    rc = rc || smk_set_sampling(ctx, sampleRate, 0, gluvv.volren.gamma, gluvv.volren.scaleAlphas);
    if (!rc) renderPresent();
    if (rc || failed) {
      std::cerr << "ERROR: HipVolumeRenderer::renderVolume: " << smk_last_error(ctx) << std::endl;
      failed = 1;
    }
    return;
  }
  fb.assign((size_t)W * H * 4, 0.0f);
  int rc = smk_set_camera(ctx, mv, gluvv.env.frustum, gluvv.env.clip, W, H);
  rc |= smk_set_sampling(ctx, sampleRate, 0, gluvv.volren.gamma, gluvv.volren.scaleAlphas);
  if (!rc) rc = smk_render(ctx, fb.data(), nullptr);
  if (rc) {
    std::cerr << "ERROR: HipVolumeRenderer::renderVolume: " << smk_last_error(ctx) << std::endl;
    failed = 1;
  }
}

void HipVolumeRenderer::renderVolume(float sampleRate, double mv[16], float xext[2], float yext[2], float zext[2]) {
  if (!ok()) return;
  // (render3DVolumeEXTSV clamps the extents to the volume and returns when nothing is left, VolumeRenderer.cpp:452-463)
  const float lo[3] = {xext[0], yext[0], zext[0]}, hi[3] = {xext[1], yext[1], zext[1]};
  if (smk_set_region(ctx, 1, lo, hi)) {
    std::cerr << "ERROR: HipVolumeRenderer::renderVolume: " << smk_last_error(ctx) << std::endl;
    failed = 1;
    return;
  }
  renderVolume(sampleRate, mv);
  smk_set_region(ctx, 0, nullptr, nullptr);
}

void HipVolumeRenderer::renderSlice(float quad[4][3], float alpha) {
  if (!ok()) return;
  const size_t npix = (size_t)gluvv.win.width * (size_t)gluvv.win.height;
  if (fb.size() != npix * 4) fb.assign(npix * 4, 0.0f);  // (no frame yet: the slice goes onto a cleared one)
  if (smk_render_slice(ctx, quad, alpha, fb.data())) {
    std::cerr << "ERROR: HipVolumeRenderer::renderSlice: " << smk_last_error(ctx) << std::endl;
    failed = 1;
  }
}

// -------------------------------------------------------------------------------------------

void HipVolumeRenderable::init() {
  if (!gluvv.mv) {  // VolumeRenderable.cpp:62-65
    std::cerr << "ERROR: HipVolumeRenderable::init(), no MetaVolume defined" << std::endl;
    return;
  }
  volren = new HipVolumeRenderer(gluvv.mv, 0, device);
  volren->useU16(u16);
  // a series keeps MetaVolume::tstepCache steps resident (MetaVolume.cpp:894-958): they are uploaded under their time-step
  // numbers from the first one on; with one step the volume is simply replaced whenever the time step moves
  tcache = gluvv.mv->tstepCache > 1 ? gluvv.mv->tstepCache : 1;
  tstep = gluvv.volren.timestep;
  int bad;
  if (tcache > 1) bad = smk_set_timestep_cache(volren->context(), tcache) || uploadStep(tstep);
  else if (gluvv.mv->numSubVols == 1) bad = volren->createVolume(VolRen3DExt, gluvv.mv->volumes);
  else bad = volren->createVolume(VolRen3DExt, gluvv.mv->volumes, gluvv.mv->numSubVols);
  if (bad || !volren->ok()) return;  // go stays 0: draw() is a no-op (NV20VolRen3D.cpp:44-65)
  if (gluvv.dmode == GDM_V1 && !gluvv.volren.deptex) {
    // scalar path: 1-D TLUT owned by the renderer, published in gluvv.volren.tlut
    // (VolumeRenderable.cpp:72-78; the preset colormaps are the caller's to choose)
    volren->createTLUT();
    gluvv.volren.tlut = volren->getColorMap();
    volren->loadTransferTableRGBA();
  } else {
    gluvv.volren.loadTLUT = 1;  // first draw() sends deptex/deptex2 (NV20VolRen3D.cpp:91-122)
  }
  createNoiseTex(32, 32, 32);  // R8kVolRen3D_cpy.cpp:61 (constructor) -> :300-304
  go = 1;
}

// R8kVolRen3D_cpy::createNoiseTex (:2392-2436): srand(1), four draws per texel, no blur pass (its
// loop runs zero times); the GL texture it fills is GL_REPEAT + GL_LINEAR -- smk_set_perturb's fetch
void HipVolumeRenderable::createNoiseTex(int sx, int sy, int sz) {
  noise.resize((size_t)sx * sy * sz * 4);
  srand(1);
  for (int i = 0; i < sz; ++i)
    for (int j = 0; j < sy; ++j)
      for (int k = 0; k < sx; ++k)
        for (int e = 0; e < 4; ++e)
          noise[(size_t)i * sx * sy * 4 + (size_t)j * sx * 4 + k * 4 + e] = (unsigned char)(((rand() / (float)RAND_MAX * .5) + .5 + 1.0 / 512) * 255);
}

void HipVolumeRenderable::modelview(double mv[16]) { build_modelview(mv); }

int HipVolumeRenderable::uploadStep(int timestep) {
  smk_ctx *c = volren ? volren->context() : nullptr;
  if (!c) return 1;
  std::vector<smk_volume_desc> d = brick_descs(gluvv.mv->volumes, gluvv.mv->numSubVols);
  if (smk_upload_timestep(c, timestep, d.data(), gluvv.mv->numSubVols, gluvv.mv->nelts, u16 ? SMK_U16 : SMK_U8, (smk_datamode)gluvv.dmode)) {
    std::cerr << "ERROR: HipVolumeRenderable: time step " << timestep << ": " << smk_last_error(c) << std::endl;
    return 1;
  }
  if (tblend_id < 0) tblend_t = -1;  // (a blend refused for want of a resident step is asked for again)
  return 0;
}

// R8kVolRen3D::renderVolume (R8kVolRen3D.cpp:184-188) rebuilds its textures from gluvv.mv when gluvv.volren.timestep moves; the
// key handler has already swapped that step into the MetaVolume or read it (gluvv.cpp:970-1010).  Here a resident step is
// selected -- no voxel moves -- and any other is uploaded from gluvv.mv's current data under its number, then selected.
int HipVolumeRenderable::showTimeStep() {
  const int t = gluvv.volren.timestep;
  smk_ctx *c = volren->context();
  if (t == tstep) {
    if (tfrac > 0) {
      showTimeFraction();
      return 0;
    }
    if (tblend_id >= 0) {  // back from a blend to the whole step, which the ring never evicts under a blend of it
      if (smk_select_timestep(c, t)) {
        std::cerr << "ERROR: HipVolumeRenderable::draw: " << smk_last_error(c) << std::endl;
        return 1;
      }
      tblend_id = -1;
    }
    tblend_t = -1;  // (the next fraction is blended afresh, one that was refused before too)
    return 0;
  }
  tblend_id = -1;  // (the whole step first: it becomes current below, then the blend from it)
  tblend_t = -1;
  if (tcache == 1) {
    const int bad = gluvv.mv->numSubVols == 1 ? volren->createVolume(VolRen3DExt, gluvv.mv->volumes)
                                              : volren->createVolume(VolRen3DExt, gluvv.mv->volumes, gluvv.mv->numSubVols);
    if (bad) return 1;
  } else if (smk_select_timestep(c, t)) {  // not cached (swapTStep's return 0)
    if (uploadStep(t)) return 1;
    if (smk_select_timestep(c, t)) {
      std::cerr << "ERROR: HipVolumeRenderable::draw: " << smk_last_error(c) << std::endl;
      return 1;
    }
  }
  tstep = t;
  if (tfrac > 0) showTimeFraction();
  return 0;
}

int HipVolumeRenderable::setTimeFraction(float f) {
  if (!(f >= 0.0f && f < 1.0f)) return 1;
  tfrac = f;
  return 0;
}

// The frames show (1 - tfrac) step tstep + tfrac step (tstep + 1), blended on the device into one of two ids no series uses,
// in turn: the slot the frame before this one reads is never the one being written.  A blend the C ABI refuses -- step
// tstep + 1 not resident -- is reported once, and the frames stay on the whole step; it is asked for again when the step or
// the fraction moves, after a fraction of 0, or after the adapter has uploaded a step.  A series cache of one step holds the
// volume and no steps (init(), showTimeStep): there is nothing to blend with, and the ring is not grown for it.
void HipVolumeRenderable::showTimeFraction() {
  if (tblend_t == tstep && tblend_f == tfrac) return;
  smk_ctx *c = volren->context();
  tblend_t = tstep;
  tblend_f = tfrac;
  if (tcache == 1) {
    std::cerr << "ERROR: HipVolumeRenderable::setTimeFraction: time step " << tstep + 1
              << " is not cached: the series keeps one step resident (MetaVolume::tstepCache < 2)" << std::endl;
    return;
  }
  const int extra = tderive ? 4 : 2;
  if (tblend_grown < extra) {
    if (smk_set_timestep_cache(c, tcache + extra)) {
      std::cerr << "ERROR: HipVolumeRenderable::setTimeFraction: " << smk_last_error(c) << std::endl;
      return;
    }
    tblend_grown = extra;
  }
  const int id = INT_MAX - tblend_next;
  int shown = id;
  const int bad = smk_blend_timesteps(c, tstep, tstep + 1, tfrac, id, nullptr);
  if (!bad && tderive) {
    // V, G, H and normals of the blended scalar -- or, for a multi-field series (gluvv.dmode GDM_V1G, GDM_V2G, GDM_V3G: what
    // mergeMV with -addG made), the blended fields with G and the normals of their summed gradient -- behind the blend on the
    // same stream: no host wait.  A refusal -- a series that is neither -- is said here, once for this step and fraction as a
    // refused blend is, and the frames show the blend
    const bool merged = gluvv.dmode == GDM_V1G || gluvv.dmode == GDM_V2G || gluvv.dmode == GDM_V3G;
    // ... and for GDM_V1GH, GDM_V2GH (mergeMV with -addH) with H of the summed gradient too, the reference's typo kept; blurred
    // normals (setBlurNormals) go to the derive and to either merge
    const bool merged_h = gluvv.dmode == GDM_V1GH || gluvv.dmode == GDM_V2GH;
    const int did = INT_MAX - 2 - tblend_next;
    // A derived id that is resident is overwritten in place.  One that is not -- its first use, or evicted since by steps the
    // series uploaded -- would take a slot by the ring's rule, which spares the derive's source and the current step but not
    // the steps tstep and tstep + 1 the NEXT fraction blends.  smk_blend_timesteps spares exactly those, so the same blend
    // into the derived id makes the id resident first, wherever the ring's turn stands
    bool resident = false;
    int n = 0;
    if (!smk_get_timesteps(c, nullptr, nullptr, 0, &n) && n > 0) {
      std::vector<int> ids((size_t)n);
      if (!smk_get_timesteps(c, nullptr, ids.data(), n, &n))
        for (int i = 0; i < n && i < (int)ids.size(); ++i) resident |= ids[(size_t)i] == did;
    }
    if (!resident && smk_blend_timesteps(c, tstep, tstep + 1, tfrac, did, nullptr))
      std::cerr << "ERROR: HipVolumeRenderable::setTimeFractionDerivatives: " << smk_last_error(c) << std::endl;
    else if (merged_h || (merged && tblur) ? smk_merge_timestep_h(c, id, did, merged_h ? 1 : 0, 1, tblur, nullptr)
             : merged                      ? smk_merge_timestep(c, id, did, nullptr)
                                           : smk_derive_timestep(c, id, did, 1, tblur, nullptr))
      std::cerr << "ERROR: HipVolumeRenderable::setTimeFractionDerivatives: " << smk_last_error(c) << std::endl;
    else
      shown = did;
  }
  if (bad || smk_select_timestep(c, shown)) {
    std::cerr << "ERROR: HipVolumeRenderable::setTimeFraction: " << smk_last_error(c) << std::endl;
    if (tblend_id >= 0 && !smk_select_timestep(c, tstep)) tblend_id = -1;
    return;
  }
  tblend_id = shown;
  tblend_next ^= 1;
}

int HipVolumeRenderable::setTimeFractionDerivatives(int on_off) {
  const int on = on_off ? 1 : 0;
  if (on != tderive) tblend_t = -1;  // (the fraction shown now is made again, with or without its derivatives)
  tderive = on;
  return 0;
}

int HipVolumeRenderable::setBlurNormals(int on_off) {
  const int on = on_off ? 1 : 0;
  if (on != tblur && tderive) tblend_t = -1;  // (the fraction shown now is made again with the other normals)
  tblur = on;
  return 0;
}

int HipVolumeRenderable::saveTimeStep(const char *prefix) {
  if (!go || !volren || !prefix) return 0;
  if (showTimeStep()) return 0;  // (the step -- or the blend -- the next draw() shows is the one that is saved)
  smk_dtype dt = SMK_U8;
  int nelts = 0;
  if (smk_get_timestep_box(volren->context(), nullptr, nullptr, &nelts, &dt, nullptr)) {
    std::cerr << "ERROR: HipVolumeRenderable::saveTimeStep: " << smk_last_error(volren->context()) << std::endl;
    return 0;
  }
  if (dt != SMK_U8) {
    std::cerr << "ERROR: HipVolumeRenderable::saveTimeStep: no 16-bit / float writer: MetaVolume::writeAll and genVGH write 8-bit voxels "
                 "(HipVolumeRenderer::downloadStep hands over the arrays)" << std::endl;
    return 0;
  }
  std::vector<unsigned char> data;
  int o[3], s[3];
  if (!volren->downloadStep(&data, nullptr, o, s)) return 0;
  // the box's extent: its share of the volume's
  const int N[3] = {gluvv.mv->xiSize, gluvv.mv->yiSize, gluvv.mv->ziSize};
  const float F[3] = {gluvv.mv->xfSize, gluvv.mv->yfSize, gluvv.mv->zfSize};
  float fs[3];
  for (int a = 0; a < 3; ++a) fs[a] = N[a] > 0 ? F[a] * (float)s[a] / (float)N[a] : F[a];
  std::string err;
  size_t w;
  if (nelts == 1) {  // writeAll: the .trex and one raw brick
    MetaVolume mv;
    Volume v;
    v.xiSize = mv.xiSize = s[0]; v.yiSize = mv.yiSize = s[1]; v.ziSize = mv.ziSize = s[2];
    v.xfSize = mv.xfSize = fs[0]; v.yfSize = mv.yfSize = fs[1]; v.zfSize = mv.zfSize = fs[2];
    v.xiPos = v.yiPos = v.ziPos = 0;
    v.xfPos = v.yfPos = v.zfPos = 0;
    v.currentData = data.data();
    mv.nelts = 1;
    mv.numSubVols = 1;
    mv.volumes = &v;
    w = smkfiles::write_trex(prefix, mv, true, &err);
    mv.volumes = nullptr;  // (both objects leave scope owning nothing)
    mv.numSubVols = 0;
    v.currentData = nullptr;
  } else {
    w = smkfiles::write_nrrd((std::string(prefix) + ".nrrd").c_str(), data.data(), nelts, s, fs, nelts == 3 ? "vgh" : "v", &err);
  }
  if (!w) {
    std::cerr << "ERROR: HipVolumeRenderable::saveTimeStep: " << err << std::endl;
    return 0;
  }
  return 1;
}

void HipVolumeRenderable::draw() {
  if (!go || !volren) return;
  if (gluvv.reblend) return;  // R8kVolRen3D.cpp:177
  if (gluvv.picking) return;  // :179
  if (showTimeStep()) {
    go = 0;
    return;
  }
  double mv[16];
  build_modelview(mv);
  smk_ctx *c = volren->context();
  if (gluvv.volren.tlut && gluvv.dmode == GDM_V1 && !gluvv.volren.deptex) {
    // VolumeRenderable::draw (:50-54): opacity-correct the TLUT for the sample rate, re-send
    // (TLUT::scaleAlpha itself re-uploads through GL and returns nothing, TLUT.h:45: the same
    //  arithmetic without the upload, then one smk_set_tlut1d when anything changed)
    if (volren->colorMap()->scaleAlphaNoUpload(gluvv.volren.sampleRate) | gluvv.volren.loadTLUT) {
      gluvv.volren.loadTLUT = 0;
      volren->loadTransferTableRGBA();
    }
  } else if (gluvv.volren.loadTLUT) {
    // TFWidgetRen raised loadTLUT after rasterising into deptex (TFWidgetRen1.cpp:232-242)
    // a table with several sheets along the third axis (gluvv.tf.ptexsz[2] > 1: what LevWidget::rasterize
    // fills as tex[h][g][v][4], LevWidget.cpp:691-693, and the old widget called ptex,
    // TFWidgetRen.cpp:779-845) is the dense 3-D transfer function; one sheet is the 2-D one x deptex2
    int bad;
    if (gluvv.tf.ptexsz[2] > 1) bad = smk_set_tf3d(c, gluvv.volren.deptex, gluvv.tf.ptexsz[0], gluvv.tf.ptexsz[1], gluvv.tf.ptexsz[2]);
    else bad = smk_set_tf2d(c, gluvv.volren.deptex, gluvv.volren.deptex2, gluvv.tf.ptexsz[0], gluvv.tf.ptexsz[1]);
    if (bad) std::cerr << "ERROR: HipVolumeRenderable::draw: " << smk_last_error(c) << std::endl;
    gluvv.volren.loadTLUT = 0;
  }
  // noise-perturbed fetch (R8kVolRen3D_cpy.cpp:300-304 constants, :1590-1595 coordinates): the _cpy
  // renderer, chosen at compile time in gluvv.cpp:164-198, always perturbs; as one renderer among the
  // others this one follows gluvv.pert.on
  if (gluvv.pert.on) smk_set_perturb(c, noise.data(), 32, gluvv.pert.weights, gluvv.pert.scales);
  else smk_set_perturb(c, nullptr, 0, nullptr, nullptr);
  // clip-plane widget, orthogonal mode (NV20VolRen3D::setupClips, NV20VolRen3D.cpp:251-327)
  smk_set_clip(c, gluvv.clip.on && gluvv.clip.ortho, (int)gluvv.clip.oaxis, gluvv.clip.vpos);
  // free mode: glClipPlane(GL_CLIP_PLANE5, {0,0,-1,0}) under wmv * T(clip.pos) * clip.xform (:346-357).
  // That matrix K is rigid, so the eye-space plane GL stores, zup * K^-1, is (-z_K, z_K . t_K): normal
  // against the widget's local z axis, through its origin.
  if (gluvv.clip.on && !gluvv.clip.ortho) {
    double wmv[16], t[16], x[16], k[16];
    build_world_modelview(wmv);
    translate(t, gluvv.clip.pos[0], gluvv.clip.pos[1], gluvv.clip.pos[2]);
    for (int i = 0; i < 16; ++i) x[i] = gluvv.clip.xform[i];
    mul(k, wmv, t);
    mul(k, k, x);
    const double plane[4] = {-k[8], -k[9], -k[10], k[8] * k[12] + k[9] * k[13] + k[10] * k[14]};
    smk_set_clip_plane(c, 1, plane);
  } else {
    smk_set_clip_plane(c, 0, nullptr);
  }
  // Phong of the platform's renderer: register combiners on the GeForce3 targets (NV20VolRen3D.cpp:634-806),
  // the cube-map shader everywhere else (R8kVolRen3D.cpp:2620-2679, 2886-2902; renderer choice gluvv.cpp:141-199)
  const bool nv20 = gluvv.plat == GPNV20 || gluvv.plat == GPNV202D;
  // the widget's data slice (drawClip, R8kVolRen3D.cpp:360-372, 400-424; NV20VolRen3D.cpp:144-148, 173-178): the corners and
  // alpha CPWidgetRen::set_info publishes, and dv = dot(normalize(eye - clip.pos), normalize(clip.dir)) as renderVolume
  // computes it (R8kVolRen3D.cpp:273-281; a widget that has not published a direction yet draws no slice).  Its colour is
  // the platform's renderer's: the NV20 final combiner, else the R8k clip shader (what gluvv.cpp:169 instantiates).
  {
    float vd[3], cd[3], lv = 0, lc = 0;
    for (int i = 0; i < 3; ++i) {
      vd[i] = gluvv.env.eye[i] - gluvv.clip.pos[i];
      cd[i] = gluvv.clip.dir[i];
      lv += vd[i] * vd[i];
      lc += cd[i] * cd[i];
    }
    lv = sqrtf(lv);
    lc = sqrtf(lc);
    const float dv = lv > 0 && lc > 0 ? (vd[0] / lv) * (cd[0] / lc) + (vd[1] / lv) * (cd[1] / lc) + (vd[2] / lv) * (cd[2] / lc) : 0.0f;
    if (smk_set_clip_slice(c, gluvv.clip.on && gluvv.clip.ortho, gluvv.clip.corners, gluvv.clip.alpha, dv,
                           nv20 ? SMK_CLIP_LOOK_NV20 : SMK_CLIP_LOOK_R8K))
      std::cerr << "ERROR: HipVolumeRenderable::draw: " << smk_last_error(c) << std::endl;
  }
  smk_shade sm = SMK_SHADE_NONE;
  if (gluvv.shade == gluvvShadeDiff) sm = nv20 ? SMK_SHADE_NV20_DIFF : SMK_SHADE_R8K_DIFF;
  if (gluvv.shade == gluvvShadeDSpec) sm = nv20 ? SMK_SHADE_NV20_DSPEC : SMK_SHADE_R8K_DSPEC;
  // gluvvShadeMIP: glBlendEquationEXT(GL_MAX) around renderBricks (NV20VolRen3D.cpp:158-163)
  smk_set_blend(c, gluvv.shade == gluvvShadeMIP ? SMK_BLEND_MAX : SMK_BLEND_FRONT_TO_BACK);
  smk_set_shading(c, sm, gluvv.light.pos, gluvv.env.eye, gluvv.env.at, gluvv.rinfo.xform, gluvv.light.intens, gluvv.light.amb);
  // shadow mode (R8kVolRen3D.cpp:296-326, 1651-1868): light buffer of buffsz texels scaled by the good or the
  // interactive quality, whichever sampling rate is in force (R8kVolRen3D::setupPBuff, :1114-1123)
  smk_set_shadow(c, gluvv.light.shadow, gluvv.light.buffsz[0],
                 gluvv.volren.sampleRate == gluvv.volren.goodSamp ? gluvv.light.gShadowQual : gluvv.light.iShadowQual);
  volren->renderVolume(gluvv.volren.sampleRate, mv);
  if (!volren->ok()) go = 0;
}

// gluLookAt(eye,at,up) * T(trans) * R(xform) * T(-size/2)   (gluvv.cpp:531-540, VolumeRenderable.cpp:40-46)
static void mul(double o[16], const double a[16], const double b[16]) {
  double t[16];
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += a[k * 4 + r] * b[c * 4 + k];
      t[c * 4 + r] = s;
    }
  memcpy(o, t, sizeof t);
}
static void translate(double m[16], double x, double y, double z) {
  memset(m, 0, 16 * sizeof(double));
  m[0] = m[5] = m[10] = m[15] = 1;
  m[12] = x; m[13] = y; m[14] = z;
}
static void build_world_modelview(double mv[16]) {  // gluLookAt(eye, at, up): the "wmv" the clip widget lives in
  const float *e = gluvv.env.eye, *a = gluvv.env.at, *u = gluvv.env.up;
  double f[3] = {a[0] - e[0], a[1] - e[1], a[2] - e[2]};
  double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  for (double &x : f) x /= fl;
  double s[3] = {f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0]};
  double sl = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
  for (double &x : s) x /= sl;
  double uu[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
  double la[16] = {s[0], uu[0], -f[0], 0, s[1], uu[1], -f[1], 0, s[2], uu[2], -f[2], 0, 0, 0, 0, 1};
  double t[16];
  translate(t, -e[0], -e[1], -e[2]);
  mul(mv, la, t);
}
static void build_modelview(double mv[16]) {
  const float *e = gluvv.env.eye, *a = gluvv.env.at, *u = gluvv.env.up;
  double f[3] = {a[0] - e[0], a[1] - e[1], a[2] - e[2]};
  double fl = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  for (double &x : f) x /= fl;
  double s[3] = {f[1] * u[2] - f[2] * u[1], f[2] * u[0] - f[0] * u[2], f[0] * u[1] - f[1] * u[0]};
  double sl = sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
  for (double &x : s) x /= sl;
  double uu[3] = {s[1] * f[2] - s[2] * f[1], s[2] * f[0] - s[0] * f[2], s[0] * f[1] - s[1] * f[0]};
  double la[16] = {s[0], uu[0], -f[0], 0, s[1], uu[1], -f[1], 0, s[2], uu[2], -f[2], 0, 0, 0, 0, 1};
  double t[16], r[16];
  translate(t, -e[0], -e[1], -e[2]);
  mul(mv, la, t);
  translate(t, gluvv.rinfo.trans[0], gluvv.rinfo.trans[1], gluvv.rinfo.trans[2]);
  mul(mv, mv, t);
  for (int i = 0; i < 16; ++i) r[i] = gluvv.rinfo.xform[i];
  mul(mv, mv, r);
  translate(t, -gluvv.mv->xfSize / 2, -gluvv.mv->yfSize / 2, -gluvv.mv->zfSize / 2);
  mul(mv, mv, t);
}
