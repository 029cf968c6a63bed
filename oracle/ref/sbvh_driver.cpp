// Builds the reference's SBVH over a triangle mesh and dumps the tree as plain
// data (oracle/ref/README.md).  Compiled with the reference's own builder
// sources against the ngl::Vec3 stand-in.
//
//   sbvh_driver <mesh.bin> <tree.bin>
//
// mesh.bin: u32 nv, nt; f32 pos[3 nv], nrm[3 nv], tan[3 nv], uv[2 nv]; u32 tris[3 nt]
// tree.bin: u32 n_nodes, n_refs
//           n_nodes x { u32 is_leaf; f32 lo[3], hi[3]; u32 a, b }   in preorder, root first;
//                      inner: a, b = node numbers of child 0 and 1; leaf: a, b = [first, last) into refs
//           u32 refs[n_refs]                                          triangle numbers
#include <cstdint>
#include <cstdio>
#include <vector>

#include "SBVH.h"

namespace
{
struct Node
{
  uint32_t isLeaf;
  float lo[3], hi[3];
  uint32_t a, b;
};

uint32_t walk(const BVHNode *_n, std::vector<Node> &_out, uint32_t &_nRefs)
{
  const uint32_t me = static_cast<uint32_t>(_out.size());
  _out.push_back(Node());
  Node rec;
  const AABB box = _n->getBounds();
  const ngl::Vec3 lo = box.minBounds(), hi = box.maxBounds();
  rec.lo[0] = lo.m_x; rec.lo[1] = lo.m_y; rec.lo[2] = lo.m_z;
  rec.hi[0] = hi.m_x; rec.hi[1] = hi.m_y; rec.hi[2] = hi.m_z;
  rec.isLeaf = _n->isLeaf() ? 1u : 0u;
  if(_n->isLeaf())
  {
    const LeafNode *leaf = static_cast<const LeafNode *>(_n);
    rec.a = leaf->firstIndex();
    rec.b = leaf->lastIndex();
    if(rec.b > _nRefs)
      _nRefs = rec.b;
  }
  else
  {
    rec.a = walk(_n->childNode(0), _out, _nRefs);
    rec.b = walk(_n->childNode(1), _out, _nRefs);
  }
  _out[me] = rec;
  return me;
}
}

int main(int argc, char **argv)
{
  if(argc != 3)
    return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if(!f)
    return 3;
  uint32_t n[2];
  bool ok = std::fread(n, 4, 2, f) == 2;
  std::vector<float> pos(3 * n[0]), nrm(3 * n[0]), tan(3 * n[0]), uv(2 * n[0]);
  std::vector<uint32_t> tris(3 * n[1]);
  ok = ok && std::fread(pos.data(), 4, pos.size(), f) == pos.size() && std::fread(nrm.data(), 4, nrm.size(), f) == nrm.size() &&
       std::fread(tan.data(), 4, tan.size(), f) == tan.size() && std::fread(uv.data(), 4, uv.size(), f) == uv.size() &&
       std::fread(tris.data(), 4, tris.size(), f) == tris.size();
  std::fclose(f);
  if(!ok)
    return 3;
  std::vector<vHVert> verts(n[0]);
  for(uint32_t i = 0; i < n[0]; ++i)
  {
    verts[i].m_vert = ngl::Vec3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]);
    verts[i].m_normal = ngl::Vec3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    verts[i].m_tangent = ngl::Vec3(tan[3 * i], tan[3 * i + 1], tan[3 * i + 2]);
    verts[i].m_u = uv[2 * i];
    verts[i].m_v = uv[2 * i + 1];
  }
  std::vector<vHTriangle> triangles(n[1]);
  for(uint32_t t = 0; t < n[1]; ++t)
    for(int k = 0; k < 3; ++k)
      triangles[t].m_indices[k] = tris[3 * t + k];

  SBVH sbvh(triangles.data(), verts.data(), n[1]);

  std::vector<Node> nodes;
  uint32_t nRefs = 0;
  walk(sbvh.getRoot(), nodes, nRefs);
  std::vector<uint32_t> refs(nRefs);
  for(uint32_t i = 0; i < nRefs; ++i)
    refs[i] = sbvh.getTriIndex(i);

  FILE *out = std::fopen(argv[2], "wb");
  if(!out)
    return 4;
  const uint32_t head[2] = { static_cast<uint32_t>(nodes.size()), nRefs };
  std::fwrite(head, 4, 2, out);
  std::fwrite(nodes.data(), sizeof(Node), nodes.size(), out);
  std::fwrite(refs.data(), 4, refs.size(), out);
  std::fclose(out);
  return 0;
}
