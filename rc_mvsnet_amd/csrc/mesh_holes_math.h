// The per-element rules of the hole-filling pass (rc_mvsnet_amd/mesh_holes.py; contract in mesh_holes.h): what a vertex's boundary
// half-edge counts make of it, what a loop of L edges adds, where its new vertex lies.  Plain C++ shared by mesh_holes.hip and
// host code, restated by tests/mesh_holes_oracle.py with the same operation order.  Floating point is fp64 under
// `fp contract(off)`.
#pragma once

#include "mesh_decimate_math.h"                                   // RCMVS_HD, mc::face_valid, md::colour

namespace rcmvs {
namespace mh {

constexpr int NONE = 0, SIMPLE = 1, COMPLEX = 2;                  // the RCMVS_MH_* values of mesh_holes.h

// out / in: the boundary half-edges that leave / arrive at the vertex
RCMVS_HD int classify(int out, int in) { return out == 1 && in == 1 ? SIMPLE : (out != 0 || in != 0 ? COMPLEX : NONE); }

// a filled loop of L >= 3 edges adds one face and no vertex (L == 3) or L faces round one new vertex
RCMVS_HD int faces_added(int L) { return L == 3 ? 1 : L; }
RCMVS_HD int verts_added(int L) { return L == 3 ? 0 : 1; }

#pragma clang fp contract(off)
// One coordinate of the new vertex: s = 0.0 + the members' coordinate, one add per member in loop order from the leader.  No
// comparison: NaN and infinities go through the arithmetic.
RCMVS_HD double add_member(double s, float p) { return s + (double)p; }
RCMVS_HD float centroid(double s, int L) { return (float)(s / (double)L); }

}  // namespace mh
}  // namespace rcmvs
