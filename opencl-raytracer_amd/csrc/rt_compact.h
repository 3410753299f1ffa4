// rt_compact.h - the host side of the compact records (rt_device.h: CompactObject): the per-object tests behind the predicate `diagonal`,
// the scene's, and the packer. Plain C++ over the ABI's byte layouts: rt_create, rt_set_transforms and the frame's switch (rt_api.cpp,
// rt_geometry.cpp, rt_context.h) call every function here, and host/compact_record_check compiles it without the library
// (tests/test_compact_records_cpu.py).
#pragma once
#include "rt_device.h"
#include "rt_records.h"

#include <cstring>

namespace rt::host {

// the off-diagonal words of the upper 3x3 of a column-major 4x4: m[4 c + r], r != c, r, c < 3
constexpr int kOffDiagonal[6] = {1, 2, 4, 6, 8, 9};

// Both upper 3x3 hold +0.0f - the bit pattern: not -0.0f, whose products differ in the sign of a zero - in every off-diagonal place.
inline bool diagonal_3x3(const float* mv, const float* mvInverse) {
    uint32_t any = 0u;
    for (int k : kOffDiagonal) {
        uint32_t a, b;
        std::memcpy(&a, mv + k, 4);
        std::memcpy(&b, mvInverse + k, 4);
        any |= a | b;
    }
    return any == 0u;
}
inline bool bottom_rows_affine(const float* mv, const float* mvInverse) {  // affine_w, per object: both bottom rows are (0,0,0,1)
    return mv[3] == 0.f && mv[7] == 0.f && mv[11] == 0.f && mv[15] == 1.f && mvInverse[3] == 0.f && mvInverse[7] == 0.f &&
           mvInverse[11] == 0.f && mvInverse[15] == 1.f;
}

// An object that keeps a scene from being diagonal by its matrices: a sphere or a box (objects of any other type are never hit and no
// kernel reads their rows; a hidden object is a sphere or a box that may be shown again, and counts by the type rt_create was given)
// whose upper 3x3 are not diagonal. What rt_create and rt_set_transforms count (rt_context: n_not_diagonal).
inline bool object_not_diagonal(uint32_t type, const float* mv, const float* mvInverse) { return type < 2u && !diagonal_3x3(mv, mvInverse); }
// The scene's predicate from what a context keeps of its objects (rt_context.h: compact_in_use): no triangle, every sphere / box affine
// (affine_w: bottom_rows_affine of each) and none of them counted by object_not_diagonal.
inline bool scene_diagonal(bool has_triangles, bool affine_w, uint32_t n_not_diagonal) { return !has_triangles && affine_w && n_not_diagonal == 0u; }

// An object's compact record: the words are moved, never computed with. Of an object that is not diagonal it holds the same six
// places of each matrix - not a faithful copy, and not read: the predicate is the scene's.
inline CompactObject pack_compact(const float* mv, const float* mvInverse, uint32_t type, float absorption) {
    CompactObject c;
    c.a0 = mvInverse[0]; c.a1 = mvInverse[5]; c.a2 = mvInverse[10];
    c.type = type;
    c.b0 = mvInverse[12]; c.b1 = mvInverse[13]; c.b2 = mvInverse[14];
    c.absorption = absorption;
    c.s0 = mv[0]; c.s1 = mv[5]; c.s2 = mv[10];
    c.pad0 = 0u;
    c.x = mv[12]; c.y = mv[13]; c.z = mv[14];
    c.spare = 0u;
    return c;
}

}  // namespace rt::host
