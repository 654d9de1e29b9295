// The per-element rules of the mesh clean-up pass (rc_mvsnet_amd/mesh_clean.py; contract in mesh_clean.h): which faces are valid,
// which components are kept, one Taubin step of one coordinate.  Plain C++ shared by mesh_clean.hip and host code, restated by
// tests/mesh_clean_oracle.py with the same operation order.  Floating point is fp64 under `fp contract(off)`.
#pragma once

#ifndef RCMVS_HD
#if defined(__HIPCC__)
#define RCMVS_HD __host__ __device__ inline
#else
#define RCMVS_HD inline
#endif
#endif

namespace rcmvs {
namespace mc {

// a face is valid when its three indices lie in [0, nv) and differ; an invalid face's indices are never used as addresses
RCMVS_HD bool face_valid(int a, int b, int c, int nv) {
    return (unsigned)a < (unsigned)nv && (unsigned)b < (unsigned)nv && (unsigned)c < (unsigned)nv && a != b && b != c && a != c;
}

// The selection rules.  max_faces: the largest component's face count; keep_largest > 0: (k_faces, k_label) is the K-th row of the
// components ordered by (faces descending, label ascending), so "among the K largest" is one comparison.
struct Select {
    int min_faces;
    double min_fraction;
    int max_faces;
    int keep_largest, k_faces, k_label;
};

#pragma clang fp contract(off)
RCMVS_HD bool keep(int faces_c, int label, const Select& s) {
    if (!(faces_c >= s.min_faces)) return false;
    if (!((double)faces_c >= s.min_fraction * (double)s.max_faces)) return false;
    if (s.keep_largest > 0 && !(faces_c > s.k_faces || (faces_c == s.k_faces && label <= s.k_label))) return false;
    return true;
}

// p' = (float)(p + f * (s / deg - p)) in fp64: s is the sum of the neighbours' coordinate (0.0, then one add per neighbour in
// ascending neighbour order).  No comparison: NaN and infinities go through the arithmetic.
RCMVS_HD float taubin(float p, double s, int deg, double f) {
    const double m = s / (double)deg;
    return (float)((double)p + f * (m - (double)p));
}

}  // namespace mc
}  // namespace rcmvs
