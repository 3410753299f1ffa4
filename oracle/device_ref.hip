// TEST INFRASTRUCTURE - not product code.
//
// Launches the reference's OpenCL-C kernels as ROCm clang builds them for gfx950 (oracle/_ref/<kernel>_gfx950.co, see
// oracle/Makefile) on the MI355X, the way the reference host does (OpenCLRaytracer.cpp:89-91: a 1-D range of
// RAYCAST_COUNT work-items in work-groups of 32). Only tests/ load this library (oracle/oracle.py DeviceReference);
// the product never does.
//
// None of the kernels bounds-checks its work-item id, so the launch covers exactly round_up(n, 32) work-items and
// every buffer they index is that long: the ray buffer is padded with copies of the last ray, the output buffer is
// pre-filled as the reference host does ({0,0,0,1} per 16-byte float3 pixel; MAX_FLOAT for hittest) and is followed
// by a 32-element canary region that is checked after the synchronise. A changed canary is an error.
//
// Argument packing (checked by oracle.py against the code object's metadata before any launch):
//   hittest(ulong count, ObjectData*, Ray*, float*)                       offsets 0 / 8 / 16 / 24
//   shade / shade_and_reflect(uint, uint, ObjectData*, uint, Light*, Ray*, float3*)
//                                                                          offsets 0 / 4 / 8 / 16 / 24 / 32 / 40
// The hidden (code-object-v5) arguments are left to the runtime.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

constexpr uint32_t kLocal = 32;
constexpr uint32_t kCanaryElems = 32;
constexpr uint32_t kCanaryWord = 0xC3A5C35Au;
constexpr size_t kObjBytes = 320, kLightBytes = 64, kRayBytes = 32;
constexpr float kMaxFloat = 3.402823466e+38F;

struct Device {
    hipModule_t mod = nullptr;
    void* objs = nullptr;
    void* lights = nullptr;
    void* rays = nullptr;
    void* out = nullptr;
    ~Device() {
        if (objs) (void)hipFree(objs);
        if (lights) (void)hipFree(lights);
        if (rays) (void)hipFree(rays);
        if (out) (void)hipFree(out);
        if (mod) (void)hipModuleUnload(mod);
    }
};

int fail(char* err, size_t err_len, const char* what, hipError_t e) {
    if (err && err_len) snprintf(err, err_len, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return (int)e ? (int)e : -1;
}

}  // namespace

#define DREF_CHECK(call)                                              \
    do {                                                              \
        hipError_t e_ = (call);                                       \
        if (e_ != hipSuccess) return fail(err, err_len, #call, e_);   \
    } while (0)

extern "C" {

int dref_local_size(void) { return (int)kLocal; }
int dref_canary_elems(void) { return (int)kCanaryElems; }

// kind 0: hittest (out: n floats), kind 1: shade / shade_and_reflect (out: n x 4 floats).
// Returns 0 on success, else a nonzero status with a message in err.
int dref_run(const void* code_object, size_t code_object_size, const char* kernel_name, int kind, uint32_t max_bounces,
             uint32_t n_objs, const void* objs, uint32_t n_lights, const void* lights, const void* rays, uint64_t n_rays,
             void* out, char* err, size_t err_len) {
    if (err && err_len) err[0] = '\0';
    if (kind != 0 && kind != 1) {
        if (err && err_len) snprintf(err, err_len, "unknown kernel kind %d", kind);
        return -1;
    }
    if (n_rays == 0) return 0;
    if (n_rays > (uint64_t)INT32_MAX - kLocal) {  // the kernels index with a signed int work-item id
        if (err && err_len) snprintf(err, err_len, "too many rays for one launch: %llu", (unsigned long long)n_rays);
        return -1;
    }
    (void)code_object_size;
    const uint64_t global = (n_rays + kLocal - 1) / kLocal * kLocal;
    const size_t elem = kind == 0 ? sizeof(float) : 4 * sizeof(float);
    const size_t words_per_elem = elem / sizeof(uint32_t);

    // host images of the padded buffers
    std::vector<unsigned char> h_rays(global * kRayBytes);
    memcpy(h_rays.data(), rays, n_rays * kRayBytes);
    for (uint64_t i = n_rays; i < global; ++i)
        memcpy(h_rays.data() + i * kRayBytes, (const unsigned char*)rays + (n_rays - 1) * kRayBytes, kRayBytes);
    const size_t out_words = (global + kCanaryElems) * words_per_elem;
    std::vector<uint32_t> h_out(out_words);
    const size_t canary_first = global * words_per_elem;
    for (uint64_t i = 0; i < global; ++i) {
        if (kind == 0) {
            memcpy(&h_out[i], &kMaxFloat, 4);
        } else {
            const float px[4] = {0.f, 0.f, 0.f, 1.f};
            memcpy(&h_out[4 * i], px, 16);
        }
    }
    for (size_t w = canary_first; w < out_words; ++w) h_out[w] = kCanaryWord;

    Device d;
    DREF_CHECK(hipModuleLoadData(&d.mod, code_object));
    hipFunction_t fn = nullptr;
    DREF_CHECK(hipModuleGetFunction(&fn, d.mod, kernel_name));

    const size_t obj_bytes = (n_objs ? n_objs : 1) * kObjBytes;
    const size_t light_bytes = (n_lights ? n_lights : 1) * kLightBytes;
    DREF_CHECK(hipMalloc(&d.objs, obj_bytes));
    DREF_CHECK(hipMalloc(&d.lights, light_bytes));
    DREF_CHECK(hipMalloc(&d.rays, h_rays.size()));
    DREF_CHECK(hipMalloc(&d.out, out_words * sizeof(uint32_t)));
    DREF_CHECK(hipMemset(d.objs, 0, obj_bytes));
    DREF_CHECK(hipMemset(d.lights, 0, light_bytes));
    if (n_objs) DREF_CHECK(hipMemcpy(d.objs, objs, n_objs * kObjBytes, hipMemcpyHostToDevice));
    if (n_lights) DREF_CHECK(hipMemcpy(d.lights, lights, n_lights * kLightBytes, hipMemcpyHostToDevice));
    DREF_CHECK(hipMemcpy(d.rays, h_rays.data(), h_rays.size(), hipMemcpyHostToDevice));
    DREF_CHECK(hipMemcpy(d.out, h_out.data(), out_words * sizeof(uint32_t), hipMemcpyHostToDevice));

    const uint32_t groups = (uint32_t)(global / kLocal);
    uint64_t count64 = n_objs;
    uint32_t mb = max_bounces, oc = n_objs, lc = n_lights;
    void* hittest_args[] = {&count64, &d.objs, &d.rays, &d.out};
    void* shade_args[] = {&mb, &oc, &d.objs, &lc, &d.lights, &d.rays, &d.out};
    DREF_CHECK(hipModuleLaunchKernel(fn, groups, 1, 1, kLocal, 1, 1, 0, nullptr, kind == 0 ? hittest_args : shade_args,
                                     nullptr));
    DREF_CHECK(hipGetLastError());
    DREF_CHECK(hipDeviceSynchronize());
    DREF_CHECK(hipMemcpy(h_out.data(), d.out, out_words * sizeof(uint32_t), hipMemcpyDeviceToHost));

    for (size_t w = canary_first; w < out_words; ++w) {
        if (h_out[w] != kCanaryWord) {
            if (err && err_len)
                snprintf(err, err_len, "canary after the output overwritten at element %zu (word 0x%08x)",
                         (w - canary_first) / words_per_elem, h_out[w]);
            return -2;
        }
    }
    memcpy(out, h_out.data(), n_rays * elem);
    return 0;
}

}  // extern "C"
