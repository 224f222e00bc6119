// HipVolumeRenderer.h -- host-side mirror of the reference renderer interface over the C ABI.
//
//   HipVolumeRenderer   same public surface as VolumeRenderer (VolumeRenderer.h:86-118):
//                       createVolume x2, createTLUT, getColorMap, renderVolume(sampleRate, mv[, x/y/zext]),
//                       renderSlice(quad, alpha), useBBox / useBBoxBrackets
//   HipVolumeRenderable a gluvvPrimitive whose init()/draw() do what VolumeRenderable (scalar,
//                       1-D TLUT; VolumeRenderable.cpp:36-82) and NV20VolRen3D/R8kVolRen3D (VGH,
//                       deptex/deptex2, Phong; NV20VolRen3D.cpp:44-185) do, minus OpenGL: the
//                       frame lands in a float RGBA buffer (premultiplied) the app can blit.
//
// Error convention of the reference: int returns 0 = ok / 1 = error, messages on cerr, a failed
// renderer turns draw() into a no-op (`go = 0`, NV20VolRen3D.cpp:44-65).  Nothing here renders
// on the CPU: without libsmk_hip.so + a HIP device init() fails and says so.
#pragma once
#include <vector>

#include "../../include/smk.h"
#include "TransferFunctions.h"  // smktf::ProbeSample (probeStep)
#ifdef SMK_USE_REFERENCE_HEADERS
#include "gluvv.h"  // the reference's own: pulls in gluvvPrimitive.h, MetaVolume.h, TLUT.h
#else
#include "gluvv_compat.h"
#endif

enum { VolRenUnkown, VolRen2DTexture, VolRen3DTexture, VolRen3DExt };  // VolumeRenderer.h:64-69

// What renderVolume / draw() leave for the host (HipVolumeRenderer::present).  The reference's frame is the 8-bit GL
// framebuffer with its depth buffer; the two present modes deliver exactly that, in pinned memory (smk.h "display-ready frames").
enum HipPresentMode {
  HipPresentFloat = 0,      // framebuffer(): premultiplied float RGBA, one call one frame (the default)
  HipPresentPipelined = 1,  // framebuffer8() [+ depthbuffer()]: a call enqueues its frame and hands over the one before it
  HipPresentSync = 2        // framebuffer8() [+ depthbuffer()]: one call one frame
};

// The renderer's colour map.  TLUT::scaleAlpha (TLUT.cpp:138-154) ends in loadTransferTableRGBA(), a
// GL colour-table upload, and returns nothing; this subclass reaches TLUT's protected members to do
// the same opacity correction on the same fields without the GL call and says whether the table
// changed (so the adapter knows when to send it through smk_set_tlut1d).  It adds no data member:
// what gluvv.volren.tlut publishes is a plain TLUT to everyone else.
class HipTLUT : public TLUT {
 public:
  HipTLUT() : TLUT() {}
  int scaleAlphaNoUpload(float sampleRate);  // 1 = alphas were rescaled
};

class HipVolumeRenderer {
 public:
  HipVolumeRenderer(MetaVolume *vm, int subVolNum, int device = 0);
  ~HipVolumeRenderer();
  int createVolume(int type, Volume *v);             // VolumeRenderer.cpp:101
  int createVolume(int type, Volume *v, int nVols);  // VolumeRenderer.cpp:128
  int createTLUT();                                  // always returns 1, as the reference (:214-219)
  TLUT *getColorMap() { return tlut; }
  HipTLUT *colorMap() { return tlut; }  // the same object with the GL-free opacity correction
  // one frame; mv = column-major modelview as glGetDoublev returns it (VolumeRenderable.cpp:47-48)
  void renderVolume(float sampleRate, double mv[16]);
  // a smaller axis-aligned box of the volume (VolumeRenderer.h:103-108): extents in volume space
  void renderVolume(float sampleRate, double mv[16], float xext[2], float yext[2], float zext[2]);
  // one textured quad blended into the frame of the last renderVolume (VolumeRenderer.h:114; camera of that call)
  void renderSlice(float quad[4][3], float alpha);
  // bounding box and brackets (VolumeRenderer.h:122-123): GL line drawing in the reference; kept so that callers
  // compile, and readable by a host that draws its own overlay
  void useBBox(int on_off) { m_bb = on_off; }
  void useBBoxBrackets(int on_off) { m_bbb = on_off; }
  // 16-bit data (no reference equivalent: the reference quantises shorts to bytes, MetaVolume.cpp:709-889).  With the switch
  // on -- before createVolume; off by default -- the Volumes' currentData is read as uint16_t voxels in host byte order
  // (VolumeFiles' load_trex with keep16) and uploaded as SMK_U16 (smk.h): nelts 1..3, normals as before.
  void useU16(int on_off) { m_u16 = on_off; }
  int u16() const { return m_u16; }
  int bbox() const { return m_bb; }
  int bboxBrackets() const { return m_bbb; }
  // the frame of the last renderVolume: [height][width][4] premultiplied float RGBA
  const float *framebuffer() const { return fb.data(); }
  // Display-ready frames.  In a present mode renderVolume fills framebuffer8() -- [height][width] RGBA8, row 0 at the bottom,
  // for glDrawPixels(w, h, GL_RGBA, GL_UNSIGNED_BYTE, ..) -- and, with depth asked for, depthbuffer() -- [height][width] float
  // window depths, 1 where the volume left nothing, for GL_DEPTH_COMPONENT / GL_FLOAT -- instead of framebuffer().  The
  // background follows gluvv.env.bgColor as display() does (gluvv.cpp:606-623): 0 composes the frame over white (alpha 255
  // everywhere), anything else leaves it premultiplied on transparent black.
  //   HipPresentPipelined: a call enqueues its frame (ray-march, conversion, copy to pinned memory) and returns the frame
  //     of the call BEFORE it, whose copy ran beside this one's ray-march: the display lags one frame, as a swap chain does.
  //     After the first call the buffers hold a cleared frame (zero bytes, depth 1).  flush() hands over the frame in
  //     flight without enqueuing another (a host that stops animating calls it, or switches to HipPresentSync).
  //   HipPresentSync: the strict one-call-one-frame behaviour.
  // The pointers stay valid until the next renderVolume / flush / present call.
  void present(HipPresentMode mode, int want_depth = 0);
  HipPresentMode presentMode() const { return pmode; }
  const unsigned char *framebuffer8() const { return fb8; }
  const float *depthbuffer() const { return zb; }
  void flush();
  int ok() const { return ctx != nullptr && !failed; }
  smk_ctx *context() { return ctx; }
  void loadTransferTableRGBA();  // what TLUT::loadTransferTableRGBA did with the GL color table
  // MetaVolume::hist2D (MetaVolume.cpp:1650-1688) for the TF window's background: 256x256 bytes, 1 = ok
  int hist2D(unsigned char *hist);
  // The same histogram of the step the frames SHOW, read from the renderer's own packed voxels (smk_hist2d_step): any voxel
  // type -- 16-bit voxels bin as floor(255 v / 65535) --, a step that was uploaded from device memory or blended in time
  // (HipVolumeRenderable::setTimeFraction), where the host holds no bytes to hand hist2D().  1 = ok, 0 with the reason on cerr
  int hist2DStep(unsigned char *hist);
  // TFWidgetRen::drawProbe's data half (TFWidgetRen1.cpp:309-595) on that step: the cell under vpos (gluvv.probe.vpos, volume
  // coordinates in [0,1]^3) fetched from the renderer (smk_probe_step) and put through smktf::probe_sample_raw -- for 8-bit
  // voxels smktf::probe_sample's results on the host's bytes, bit for bit.  1 = *out is filled (out->inside 0 outside the
  // volume, as probe_sample leaves it); 0 with the reason on cerr when the fetch fails or this context does not hold the cell
  int probeStep(const float vpos[3], smktf::ProbeSample *out);
  // The voxels of the step the frames SHOW, read back from the renderer (smk_download_timestep): what Volume::writeVol
  // (MetaVolume.cpp:99-126) takes from currentData / currentGrad, for a step the host holds no array of -- one that was
  // blended in time or uploaded from device memory.  data: [sz][sy][sx][nelts] of the step's type (unsigned char, or
  // uint16_t with useU16), sized in BYTES; grad_or_null: [sz][sy][sx][3] normal bytes, 128s when the volume has none;
  // origin / size (either may be null): the box that came back, in voxels (x, y, z) -- the whole volume unless the context is
  // a shard.  1 = ok, 0 with the reason on cerr
  int downloadStep(std::vector<unsigned char> *data, std::vector<unsigned char> *grad_or_null, int origin[3], int size[3]);

 private:
  int upload(Volume *v, int n);
  smk_ctx *ctx;
  MetaVolume *m_vol;
  HipTLUT *tlut;
  std::vector<float> fb;
  void renderPresent();                   // renderVolume's frame in a present mode (camera and sampling already set)
  int endTicket();                        // the frame in flight becomes framebuffer8() / depthbuffer()
  HipPresentMode pmode;
  int pdepth;
  long long pticket;                      // the frame in flight (0: none)
  int pW, pH;                             // ... and the window it was enqueued with
  const unsigned char *fb8;
  const float *zb;
  std::vector<unsigned char> blank8;      // what framebuffer8() / depthbuffer() hold before the first frame arrives
  std::vector<float> blankz;
  int failed;
  int m_bb;
  int m_bbb;
  int m_u16;
};

class HipVolumeRenderable final : public gluvvPrimitive {
 public:
  explicit HipVolumeRenderable(int device = 0)
      : volren(nullptr), go(0), device(device), tstep(0), tcache(1), u16(0), tfrac(0), tblend_t(-1), tblend_f(0), tblend_id(-1), tblend_next(0),
        tblend_grown(0), tderive(0), tblur(0) {}
  ~HipVolumeRenderable() { delete volren; }  // (gluvvPrimitive's destructor is not virtual, gluvvPrimitive.h:26: delete through this type)
  void init();  // virtual in gluvvPrimitive (gluvvPrimitive.h:29-30)
  void draw();
  const float *framebuffer() const { return volren ? volren->framebuffer() : nullptr; }
  // display-ready frames (HipVolumeRenderer::present): call after init().  draw() then fills framebuffer8() and, with
  // want_depth, depthbuffer(); in HipPresentPipelined mode draw() enqueues its frame and hands over the one before it, so
  // after draw() framebuffer8() holds the newest FINISHED frame; HipPresentSync is one draw() one frame.
  void present(HipPresentMode mode, int want_depth = 0) { if (volren) volren->present(mode, want_depth); }
  const unsigned char *framebuffer8() const { return volren ? volren->framebuffer8() : nullptr; }
  const float *depthbuffer() const { return volren ? volren->depthbuffer() : nullptr; }
  void flush() { if (volren) volren->flush(); }
  void useU16(int on_off) { u16 = on_off; }  // before init(): gluvv.mv holds uint16_t voxels (HipVolumeRenderer::useU16)
  // fractional time (an extension, like useU16: the reference shows whole steps).  With f in (0, 1) draw() shows the blend of
  // the steps gluvv.volren.timestep and timestep + 1 at weight f (smk_blend_timesteps), which both have to be resident; f == 0
  // is the whole step, as before.  Returns 1 for an f outside [0, 1).  Call after init().  The series must keep at least two
  // steps resident (gluvv.mv->tstepCache >= 2); a blend that is refused -- step timestep + 1 not resident -- is reported once
  // on stderr and the frames stay on the whole step until the step or the fraction moves.
  int setTimeFraction(float f);
  // derivatives of the blend (an extension beside setTimeFraction).  On: the frames of a fraction show not the blend -- whose G
  // and H are the blends of G and H -- but the VGH step of the blended SCALAR, channel 0 of the blend: makeVGH's V, G, H (the
  // reference's h[4] typo kept) and normalsVGH's plain normals, made on the device by smk_derive_timestep into a second pair
  // of reserved ids; the ring grows by two more slots.  A multi-field series -- gluvv.dmode GDM_V1G, GDM_V2G or GDM_V3G, what
  // MetaVolume::mergeMV with -addG made of one to three fields -- shows the merged step of the blended FIELDS instead: the fields
  // as blended, G of their summed gradient and its normals (smk_merge_timestep), by the same ids and rules.  Every other series
  // must be V, G, H (nelts 3): a derive that is refused is reported once on stderr, as a refused blend is, and the frames show
  // the blend.  Returns 0.  Call after init().
  int setTimeFractionDerivatives(int on_off);
  // gluvv.cpp's file-scope `blurnorms` (-blurNormals, gluvv.cpp:1457), which initData() hands to normalsVGH and mergeMV.
  // Default 0.  On: the derivatives of a blend carry blurred normals, in the derive and in the merge.  A series of data mode
  // GDM_V1GH or GDM_V2GH -- what mergeMV with -addH made of one or two fields -- shows under setTimeFractionDerivatives the
  // blended fields with G AND H of their summed gradient (smk_merge_timestep_h, add_h 1, the reference's typo kept).  With
  // this unset and the other data modes the calls are those described above.  Returns 0.  Call after init().
  int setBlurNormals(int on_off);
  // MetaVolume::writeAll + Volume::writeVol (MetaVolume.cpp:99-126, 963-1000) for the step draw() shows -- a blend made by
  // setTimeFraction included --, read back from the renderer (HipVolumeRenderer::downloadStep).  A one-channel 8-bit step
  // goes to "<prefix>.trex" plus the raw brick, one sub-volume, as writeAll writes it (smkfiles::write_trex); a
  // multi-channel 8-bit step to "<prefix>.nrrd" (smkfiles::write_nrrd, genVGH's writer).  16-bit and float steps are
  // refused -- no 16-bit / float writer exists --: their arrays are downloadStep's.  Call after init().  1 = written, 0 with
  // the reason on cerr
  int saveTimeStep(const char *prefix);
  int running() const { return go; }
  HipVolumeRenderer *renderer() { return volren; }  // the inner interface (VolumeRenderable keeps it private; a host that
                                                    // draws sub-boxes or slice quads needs it)
  static void modelview(double mv[16]);             // what draw() hands renderVolume: LookAt * T(trans) * R(xform) * T(-fSize/2)

 private:
  void createNoiseTex(int sx, int sy, int sz);  // R8kVolRen3D_cpy::createNoiseTex (:2392-2436)
  int uploadStep(int timestep);                 // gluvv.mv's current data as that time step (smk_upload_timestep)
  int showTimeStep();                           // R8kVolRen3D::renderVolume's time-step check (R8kVolRen3D.cpp:184-188)
  HipVolumeRenderer *volren;
  int go;
  int device;
  int tstep;   // the time step the frames show (gluvv.volren.timestep when it was uploaded or selected)
  int tcache;  // device-resident steps: gluvv.mv->tstepCache, at least 1
  int u16;     // gluvv.mv's voxels are uint16_t and go up as SMK_U16 (useU16)
  void showTimeFraction();  // the blend of (tstep, tstep + 1) at tfrac, made again only when one of the two changed
  float tfrac;              // setTimeFraction
  int tblend_t;             // the (time step, fraction) of the last blend asked for, made or refused (-1: none)
  float tblend_f;
  int tblend_id;            // the reserved id the frames show instead of tstep (-1: they show tstep)
  int tblend_next;          // which of the two reserved ids, INT_MAX and INT_MAX - 1, the next blend goes into (its derived
                            // step: INT_MAX - 2 and INT_MAX - 3)
  int tblend_grown;         // the slots the ring has beyond the series': 2 that the blends live in, 4 with their derived steps
  int tderive;              // setTimeFractionDerivatives
  int tblur;                // setBlurNormals
  std::vector<unsigned char> noise;  // [sz][sy][sx][4]
};
