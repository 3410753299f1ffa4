// compact_record_check - the compact records of scale-and-translate scenes (csrc/rt_device.h: CompactObject, csrc/rt_compact.h) on the
// host: no library, no GPU (tests/test_compact_records_cpu.py).
//
//   compact_record_check <n_objects> <seed>
//
// 1. The predicate, from the functions of rt_compact.h that rt_create, rt_set_transforms and the frame's switch call (the same predicate
//    on live contexts, through rt_get_compact_info: tests/test_compact_records_gpu.py): a seeded scene of
//    non-uniformly scaled, translated spheres and boxes is diagonal; one rotated instance, a -0.0f or a NaN in an off-diagonal place
//    of either matrix, a triangle, or a bottom row that is not (0,0,0,1) each make it not; an object of a type that is never hit does not count.
// 2. The packer: the rows compact_inv_rows / compact_mv_rows rebuild from pack_compact's record are, word for word, the rows the
//    full records hold (HotObject::row0..2 = ObjectRecord::inv_row, ColdObject::mv_row[0..2] = ObjectRecord::mv_row: row r of a
//    column-major matrix is words r, 4 + r, 8 + r, 12 + r), with the type and the absorption.
// 3. The reader: materialise_frame() from the compact table gives the HitRec, the ObjRows and the absorption it gives from the full
//    records, word for word, in the three arithmetic modes, for seeded rays with zero, denormal, infinite and NaN components among them
//    (one NaN payload throughout: generated_nan below says why).
//
// rt_device.h is device code, compiled here for the host as reflection_record_check.cpp does.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
static inline float host_frexp_mant(float x) { int e; return std::frexp(x, &e); }
static inline int host_frexp_exp(float x) { int e; (void)std::frexp(x, &e); return e; }
#define __builtin_amdgcn_rcpf(x) (1.0f / (x))
#define __builtin_amdgcn_rsqf(x) (1.0f / std::sqrt(x))
#define __builtin_amdgcn_sqrtf(x) (std::sqrt(x))
#define __builtin_amdgcn_frexp_mantf(x) host_frexp_mant(x)
#define __builtin_amdgcn_frexp_expf(x) host_frexp_exp(x)
#define __builtin_amdgcn_exp2f(x) (std::exp2(x))
#define __builtin_amdgcn_logf(x) (std::log2(x))
#include "rt_compact.h"

namespace {

uint64_t rng_state;
uint32_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
float from_bits(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
float uniform(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffffffu) * (1.0f / 16777216.0f); }

// mv = T * S and its inverse, column-major; scales of either sign, never near zero
rt_object_data diagonal_object(uint32_t type) {
    rt_object_data o;
    std::memset(&o, 0, sizeof(o));
    for (int a = 0; a < 3; ++a) {
        const float s = uniform(0.2f, 3.0f) * ((rnd() & 7u) == 0u ? -1.0f : 1.0f), t = uniform(-40.f, 40.f);
        o.mv[5 * a] = s;
        o.mv[12 + a] = t;
        o.mvInverse[5 * a] = 1.0f / s;
        o.mvInverse[12 + a] = -t / s;
    }
    o.mv[15] = 1.0f;
    o.mvInverse[15] = 1.0f;
    o.type = type;
    o.mat.absorption = uniform(0.f, 1.f);
    return o;
}

std::vector<rt_object_data> diagonal_scene(uint32_t n) {
    std::vector<rt_object_data> objs(n);
    for (uint32_t i = 0; i < n; ++i) objs[i] = diagonal_object(rnd() & 1u);
    return objs;
}

// The scene's predicate over an object array, put together as rt_create puts it together, from the functions it calls: a triangle,
// bottom_rows_affine of every sphere / box (affine_w), object_not_diagonal counted (n_not_diagonal), scene_diagonal of the three.
bool scene_diagonal(const rt_object_data* objs, uint32_t n) {
    bool has_triangles = false, affine_w = true;
    uint32_t n_not_diagonal = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const rt_object_data& o = objs[i];
        has_triangles = has_triangles || o.type == 2u;
        if (o.type < 2u) affine_w = affine_w && rt::host::bottom_rows_affine(o.mv, o.mvInverse);
        n_not_diagonal += rt::host::object_not_diagonal(o.type, o.mv, o.mvInverse) ? 1u : 0u;
    }
    return rt::host::scene_diagonal(has_triangles, affine_w, n_not_diagonal);
}

int check_predicate(uint32_t n) {
    const std::vector<rt_object_data> base = diagonal_scene(n);
    const bool diagonal = scene_diagonal(base.data(), n);
    auto with = [&](auto change) {
        std::vector<rt_object_data> objs = base;
        change(objs[rnd() % n]);
        return scene_diagonal(objs.data(), n);
    };
    const bool rotated = with([](rt_object_data& o) {  // a quarter turn about z: the instance is still a box, the matrices are not diagonal
        const float c = 0.8f, s = 0.6f;
        o.mv[0] = c; o.mv[1] = s; o.mv[4] = -s; o.mv[5] = c;
        o.mvInverse[0] = c; o.mvInverse[1] = -s; o.mvInverse[4] = s; o.mvInverse[5] = c;
    });
    bool neg_zero = false, nan = false;
    for (int k : rt::host::kOffDiagonal)
        for (int which = 0; which < 2; ++which) {
            neg_zero = neg_zero || with([&](rt_object_data& o) { (which ? o.mvInverse : o.mv)[k] = -0.0f; });
            nan = nan || with([&](rt_object_data& o) { (which ? o.mvInverse : o.mv)[k] = from_bits(0x7fc00000u); });
        }
    const bool triangle = with([](rt_object_data& o) { o.type = 2u; });
    bool not_affine = false;
    for (int k : {3, 7, 11})
        for (int which = 0; which < 2; ++which)
            not_affine = not_affine || with([&](rt_object_data& o) { (which ? o.mvInverse : o.mv)[k] = 0.25f; });
    not_affine = not_affine || with([](rt_object_data& o) { o.mv[15] = 2.0f; });
    // a type that is never hit: its rows are read by no kernel
    const bool never_hit = with([](rt_object_data& o) { o.type = 7u; o.mv[1] = 0.5f; });
    std::printf("predicate diagonal %d rotated %d neg_zero %d nan %d triangle %d not_affine %d never_hit %d\n", (int)diagonal, (int)rotated,
                (int)neg_zero, (int)nan, (int)triangle, (int)not_affine, (int)never_hit);
    return (diagonal && !rotated && !neg_zero && !nan && !triangle && !not_affine && never_hit) ? 0 : 1;
}

float4 row_of(const float* m, int r) { return make_float4(m[r], m[4 + r], m[8 + r], m[12 + r]); }
bool same(const float4& a, const float4& b) { return std::memcmp(&a, &b, 16) == 0; }

unsigned long long check_packer(const std::vector<rt_object_data>& objs) {
    unsigned long long bad = 0;
    for (const rt_object_data& o : objs) {
        const rt::CompactObject c = rt::host::pack_compact(o.mv, o.mvInverse, o.type, o.mat.absorption);
        float4 r0, r1, r2, m0, m1, m2;
        uint32_t type;
        float absorption;
        rt::compact_inv_rows(&c, r0, r1, r2, type, &absorption);
        rt::compact_mv_rows(&c, m0, m1, m2);
        const bool ok = same(r0, row_of(o.mvInverse, 0)) && same(r1, row_of(o.mvInverse, 1)) && same(r2, row_of(o.mvInverse, 2)) &&
                        same(m0, row_of(o.mv, 0)) && same(m1, row_of(o.mv, 1)) && same(m2, row_of(o.mv, 2)) && type == o.type &&
                        std::memcmp(&absorption, &o.mat.absorption, 4) == 0;
        bad += ok ? 0u : 1u;
    }
    std::printf("packer objects %zu mismatches %llu\n", objs.size(), bad);
    return bad;
}

// The NaN this machine's arithmetic generates. Every NaN below is this one: where an operation meets two NaNs the hardware hands on one
// operand's payload, which operand comes first is the compiler's choice per code path, and with one payload that choice cannot show.
// (The GPU's frames are in the same position: their NaNs are all generated, none is a caller's.)
float generated_nan() {
    volatile float zero = 0.0f;
    return zero / zero;
}
// one ray component of a given kind: 0 ordinary, 1 zero (either sign), 2 denormal, 3 NaN, 4 infinity, 5 huge
float component(uint32_t kind) {
    switch (kind) {
        case 1: return from_bits(rnd() & 0x80000000u);
        case 2: return from_bits((rnd() & 0x80000000u) | (1u + (rnd() & 0x7ffffeu)));
        case 3: return generated_nan();
        case 4: return from_bits((rnd() & 0x80000000u) | 0x7f800000u);
        case 5: return uniform(-1.f, 1.f) * 3.0e37f;
        default: return uniform(-50.f, 50.f);
    }
}

template <int AM>
unsigned long long check_reader(const std::vector<rt_object_data>& objs, const char* name) {
    const size_t n = objs.size();
    // the tables as rt_create lays them out: the compact records behind the n + 1 HotObjects
    std::vector<rt::HotObject> hot(2 * (n + 1));
    std::vector<rt::ObjectRecord> rec(n);
    std::vector<rt::ColdObject> cold(n);
    std::memset(hot.data(), 0, sizeof(rt::HotObject) * hot.size());
    std::memset(rec.data(), 0, sizeof(rt::ObjectRecord) * n);
    std::memset(cold.data(), 0, sizeof(rt::ColdObject) * n);
    rt::CompactObject* compact = reinterpret_cast<rt::CompactObject*>(hot.data() + n + 1);
    for (size_t i = 0; i < n; ++i) {
        const rt_object_data& o = objs[i];
        for (int r = 0; r < 3; ++r) {
            (&hot[i].row0)[r] = row_of(o.mvInverse, r);
            rec[i].inv_row[r] = row_of(o.mvInverse, r);
            rec[i].mv_row[r] = row_of(o.mv, r);
        }
        for (int r = 0; r < 4; ++r) cold[i].mv_row[r] = row_of(o.mv, r);
        cold[i].inv_row3 = row_of(o.mvInverse, 3);
        hot[i].type = rec[i].type = o.type;
        rec[i].absorption = o.mat.absorption;
        compact[i] = rt::host::pack_compact(o.mv, o.mvInverse, o.type, o.mat.absorption);
    }
    rt::Scene S;
    std::memset(&S, 0, sizeof(S));
    S.hot = hot.data();
    S.objrec = rec.data();
    S.cold = cold.data();
    S.n_objs = (uint32_t)n;
    S.affine = 1u;
    S.diagonal = 1u;
    unsigned long long bad = 0, nan_hits = 0;
    if (rt::compact_table(S) != compact) ++bad;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t plan = (uint32_t)i & 3u;  // every fourth ray is ordinary throughout
        rt::Ray ray;
        float* w[6] = {&ray.sx, &ray.sy, &ray.sz, &ray.dx, &ray.dy, &ray.dz};
        for (float* p : w) *p = component(plan == 0u ? 0u : rnd() % 6u);
        ray.sw = 1.0f;
        ray.dw = 0.0f;
        const float t = plan == 3u ? component(rnd() % 6u) : uniform(0.f, 80.f);
        rt::HitRec full, small;
        rt::ObjRows rows_full, rows_small;
        float a_full = -1.f, a_small = -2.f;
        std::memset(&full, 0, sizeof(full)); std::memset(&small, 0, sizeof(small));
        std::memset(&rows_full, 0, sizeof(rows_full)); std::memset(&rows_small, 0, sizeof(rows_small));
        rt::materialise_frame<AM>(S, nullptr, (int)i, t, ray, full, rows_full, a_full);
        rt::materialise_frame<AM>(S, compact, (int)i, t, ray, small, rows_small, a_small);
        const bool ok = std::memcmp(&full, &small, sizeof(full)) == 0 && std::memcmp(&rows_full, &rows_small, sizeof(rows_full)) == 0 &&
                        std::memcmp(&a_full, &a_small, 4) == 0;
        bad += ok ? 0u : 1u;
        if (full.px != full.px || full.nx != full.nx) ++nan_hits;
    }
    std::printf("%s hits %zu nan_hits %llu mismatches %llu\n", name, n, nan_hits, bad);
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: compact_record_check <n_objects> <seed>\n"); return 2; }
    const uint32_t n = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    rng_state = std::strtoull(argv[2], nullptr, 10);
    if (n == 0) return 2;
    unsigned long long bad = (unsigned long long)check_predicate(n);
    const std::vector<rt_object_data> objs = diagonal_scene(n);
    bad += check_packer(objs);
    bad += check_reader<rt::kUnfused>(objs, "unfused");
    bad += check_reader<rt::kFused>(objs, "fused");
    bad += check_reader<rt::kDeviceCL>(objs, "device_opencl");
    return bad ? 1 : 0;
}
