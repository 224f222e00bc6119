// Drives HipVolumeRenderable with the clip-plane widget in orthogonal mode, the way Simian's display() finds it after
// CPWidgetRen::set_info (CPWidgetRen.cpp:215-296) published the plane: gluvv.clip.{on, ortho, oaxis, vpos, corners, alpha,
// pos, dir}.  One init(), one draw(), the frame written as floats.
// usage: clip_slice_main <vol.u8> <nx> <ny> <nz> <nelts> <grad.u8|-> <deptex.rgba> <W> <H> <rate> <shade> <xform16...> <out.f32>
//        then key=value: on= ortho= oaxis= alpha= vpos=x,y,z pos=x,y,z dir=x,y,z corners=<12 floats> plat=<gluvvPlatform>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "HipVolumeRenderer.h"

gluvvGlobal gluvv;

static std::vector<unsigned char> slurp(const char *p) {
  std::vector<unsigned char> v;
  FILE *f = fopen(p, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  v.resize(n);
  if (fread(v.data(), 1, n, f) != (size_t)n) v.clear();
  fclose(f);
  return v;
}

int main(int argc, char **argv) {
  if (argc < 12 + 16) {
    fprintf(stderr, "bad usage\n");
    return 2;
  }
  gluvvCompatDefaults(gluvv);
  int a = 1;
  auto vol = slurp(argv[a++]);
  int nx = atoi(argv[a++]), ny = atoi(argv[a++]), nz = atoi(argv[a++]), ne = atoi(argv[a++]);
  auto grad = slurp(argv[a++]);
  auto dep = slurp(argv[a++]);
  gluvv.win.width = atoi(argv[a++]);
  gluvv.win.height = atoi(argv[a++]);
  gluvv.volren.sampleRate = (float)atof(argv[a++]);
  gluvv.shade = (gluvvShade)atoi(argv[a++]);
  for (int i = 0; i < 16; ++i) gluvv.rinfo.xform[i] = (float)atof(argv[a++]);
  const char *out = argv[a++];
  for (; a < argc; ++a) {
    const std::string kv = argv[a];
    const size_t eq = kv.find('=');
    if (eq == std::string::npos) continue;
    const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
    float *c = &gluvv.clip.corners[0][0];
    if (k == "on") gluvv.clip.on = atoi(v.c_str());
    else if (k == "ortho") gluvv.clip.ortho = atoi(v.c_str());
    else if (k == "oaxis") gluvv.clip.oaxis = (VolRenMajorAxis)atoi(v.c_str());
    else if (k == "alpha") gluvv.clip.alpha = (float)atof(v.c_str());
    else if (k == "plat") gluvv.plat = (gluvvPlatform)atoi(v.c_str());
    else if (k == "vpos") sscanf(v.c_str(), "%f,%f,%f", &gluvv.clip.vpos[0], &gluvv.clip.vpos[1], &gluvv.clip.vpos[2]);
    else if (k == "pos") sscanf(v.c_str(), "%f,%f,%f", &gluvv.clip.pos[0], &gluvv.clip.pos[1], &gluvv.clip.pos[2]);
    else if (k == "dir") sscanf(v.c_str(), "%f,%f,%f", &gluvv.clip.dir[0], &gluvv.clip.dir[1], &gluvv.clip.dir[2]);
    else if (k == "corners")
      sscanf(v.c_str(), "%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f,%f", c, c + 1, c + 2, c + 3, c + 4, c + 5, c + 6, c + 7, c + 8, c + 9, c + 10, c + 11);
  }
  if (vol.size() != (size_t)nx * ny * nz * ne || dep.empty()) {
    fprintf(stderr, "volume size mismatch or no table\n");
    return 2;
  }
  MetaVolume mv;
  Volume v;
  int mx = nx > ny ? (nx > nz ? nx : nz) : (ny > nz ? ny : nz);
  mv.xiSize = v.xiSize = nx; mv.yiSize = v.yiSize = ny; mv.ziSize = v.ziSize = nz;
  mv.xfSize = v.xfSize = nx / (float)mx; mv.yfSize = v.yfSize = ny / (float)mx; mv.zfSize = v.zfSize = nz / (float)mx;
  v.currentData = vol.data();
  v.currentGrad = grad.empty() ? nullptr : grad.data();
  mv.volumes = &v;
  mv.numSubVols = 1;
  mv.nelts = ne;
  gluvv.mv = &mv;
  gluvv.dmode = GDM_VGH;
  const float fr = 0.5f / 7;
  gluvv.env.frustum[0] = -fr; gluvv.env.frustum[1] = fr; gluvv.env.frustum[2] = -fr; gluvv.env.frustum[3] = fr;
  gluvv.volren.deptex = dep.data();

  gluvvPrimitive renderables;
  HipVolumeRenderable *r = new HipVolumeRenderable(0);
  renderables.setNext(r);
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->init();
  if (!r->running()) {
    fprintf(stderr, "renderer did not start (no HIP device?)\n");
    return 3;
  }
  for (gluvvPrimitive *p = renderables.getNext(); p; p = p->getNext()) p->draw();
  if (!r->running()) return 4;
  FILE *f = fopen(out, "wb");
  fwrite(r->framebuffer(), 4, (size_t)gluvv.win.width * gluvv.win.height * 4, f);
  fclose(f);
  delete r;
  return 0;
}
