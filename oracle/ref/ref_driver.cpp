// Renders a scene blob with the reference path tracer compiled for the host
// (oracle/ref/README.md).  The scene is set up through the reference's own
// host entry points only, in the order its renderer class calls them, and
// rendered one cu_runRenderKernel call per frame, frames numbered 1..N.
//
//   ref_driver <scene.blob> <out.bin>
//
// scene.blob (little endian; written by oracle/pyoracle.py write_ref_blob):
//   u32 magic 'VRB1', W, H, frames, cornell, example_sphere, view_brdf
//   f32 origin[3], dir[3], up[3], right[3], fov_scale, fresnel_coef, fresnel_pow
//   u32 times[frames]
//   u32 n_bvh_f4, n_slots; f32 bvh[4 n_bvh_f4], verts[4 n], normals[4 n], tangents[4 n], uvs[2 n]
//   u32 hdr_w, hdr_h; f32 hdr[4 w h]
//   3 x (u32 w, h; f32 texels[4 w h])          diffuse, normal, specular
//   u32 has_brdf; f32 table[3 * 90 * 90 * 180]
// out.bin: f32 accum[4 W H]; u8 rgba[4 W H]; u8 depth[4 W H]
#include <vector>

#include <cuda_runtime.h>

#include "PathTracer.cuh"

namespace
{
struct Reader
{
  FILE *f;
  bool ok = true;
  template <typename T> T get()
  {
    T v{};
    ok = ok && std::fread(&v, sizeof(T), 1, f) == 1;
    return v;
  }
  template <typename T> void get(std::vector<T> &dst) { ok = ok && std::fread(dst.data(), sizeof(T), dst.size(), f) == dst.size(); }
};

float4 readVec(Reader &in)
{
  const float x = in.get<float>(), y = in.get<float>(), z = in.get<float>();
  return make_float4(x, y, z, 0.f);
}
}

int main(int argc, char **argv)
{
  if(argc != 3)
  {
    std::fprintf(stderr, "usage: ref_driver <scene.blob> <out.bin>\n");
    return 2;
  }
  Reader in{ std::fopen(argv[1], "rb") };
  if(!in.f || in.get<uint32_t>() != 0x31425256u)
    return 3;
  const uint32_t W = in.get<uint32_t>(), H = in.get<uint32_t>(), frames = in.get<uint32_t>();
  const bool cornell = in.get<uint32_t>() != 0, example = in.get<uint32_t>() != 0, viewBrdf = in.get<uint32_t>() != 0;
  vCamera cam;
  cam.m_origin = readVec(in);
  cam.m_dir = readVec(in);
  cam.m_upV = readVec(in);
  cam.m_rightV = readVec(in);
  cam.m_fovScale = in.get<float>();
  const float fresnelCoef = in.get<float>(), fresnelPow = in.get<float>();
  std::vector<uint32_t> times(frames);
  in.get(times);

  const uint32_t nBvh = in.get<uint32_t>(), nSlots = in.get<uint32_t>();
  std::vector<float4> bvh(nBvh), verts(nSlots), normals(nSlots), tangents(nSlots);
  std::vector<float2> uvs(nSlots);
  in.get(bvh); in.get(verts); in.get(normals); in.get(tangents); in.get(uvs);

  const uint32_t hdrW = in.get<uint32_t>(), hdrH = in.get<uint32_t>();
  std::vector<float4> hdr((size_t)hdrW * hdrH);
  in.get(hdr);

  std::vector<float4> tex[3];
  uint32_t texW[3], texH[3];
  for(int t = 0; t < 3; ++t)
  {
    texW[t] = in.get<uint32_t>(); texH[t] = in.get<uint32_t>();
    tex[t].resize((size_t)texW[t] * texH[t]);
    in.get(tex[t]);
  }
  std::vector<float> brdf;
  if(in.get<uint32_t>() != 0)
  {
    brdf.resize(3u * 90u * 90u * 180u);
    in.get(brdf);
  }
  std::fclose(in.f);
  if(!in.ok)
    return 3;

  // scene state, through the reference's host entry points
  cu_useCornellBox(cornell);
  cu_useExampleSphere(example);
  if(nSlots)
    cu_meshInitialised();
  if(!hdr.empty())
    cu_setHDRDim(hdrW, hdrH);
  const vTextureType kinds[3] = { DIFFUSE, NORMAL, SPECULAR };
  for(int t = 0; t < 3; ++t)
    if(!tex[t].empty())
      cu_bindTexture(tex[t].data(), texW[t], texH[t], kinds[t]);
  if(!brdf.empty())
    cu_bindBRDF(brdf.data());
  cu_useBRDF(viewBrdf);

  std::vector<float4> accum((size_t)W * H, make_float4(0.f, 0.f, 0.f, 0.f));
  std::vector<uchar4> rgba((size_t)W * H, make_uchar4(0, 0, 0, 0)), depth((size_t)W * H, make_uchar4(0, 0, 0, 0));
  vro_ref::Surface colourSurface = { rgba.data(), W, H }, depthSurface = { depth.data(), W, H };
  cu_fillFloat4(accum.data(), make_float4(0.f, 0.f, 0.f, 0.f), W * H);

  for(uint32_t f = 0; f < frames; ++f)
    cu_runRenderKernel(vro_ref::surfaceHandle(&colourSurface), vro_ref::surfaceHandle(&depthSurface),
                       hdr.empty() ? nullptr : hdr.data(), verts.data(), normals.data(), tangents.data(), bvh.data(),
                       uvs.data(), accum.data(), cam, W, H, f + 1, times[f], fresnelCoef, fresnelPow);
  cu_cleanUp();

  FILE *out = std::fopen(argv[2], "wb");
  if(!out)
    return 4;
  std::fwrite(accum.data(), sizeof(float4), accum.size(), out);
  std::fwrite(rgba.data(), sizeof(uchar4), rgba.size(), out);
  std::fwrite(depth.data(), sizeof(uchar4), depth.size(), out);
  std::fclose(out);
  return 0;
}
