// gather_rate.hip's question, asked of the WAVE-COOPERATIVE form of the same fetch: every lane of a wave wants some 16-byte chunks
// of its own random 128-byte record. Per lane (gather_rate.hip, repeated here for the same run): one dwordx4 load per chunk, each
// 64-way divergent. Cooperative: LPR (8 or 4) neighbouring lanes fetch consecutive chunks of ONE record - lane l loads chunk l % LPR
// of the record wanted by lane (64 / LPR) * j + l / LPR, j = 0 .. LPR-1 - so a wave instruction touches 64 / LPR lines instead of
// up to 64, and every lane gets its own record's chunks back through an LDS transposition (ds_write_b128, wave barrier,
// ds_read_b128). The staging image is swizzled: chunk c of staged record r sits at position c ^ ((r / (16 / LPR)) % LPR) of its
// row, which makes the 16 lanes of every ds_read_b128 lane group cover the 64 banks once (rows are LPR * 16 bytes, lane l reads
// row l) and leaves each ds_write_b128 group of 8 lanes inside whole rows.
//   CHUNKS  chunks of the record a lane needs: 8 (all), 7 (chunks 0..6: an ObjectRecord without its last row), 3 (chunks 4..6:
//           three material words in the upper half of a ColdObject). All LPR lanes of a record load and stage their chunk, wanted
//           or not - the line is touched anyway, and a load under a lane condition made the compiler keep the loaded chunks in
//           scratch memory (27 CU-cycles per lane-record) - so CHUNKS only sets how many chunks a lane reads back.
//   STAGE   lanes staged at a time: 64 (8 KB per wave at LPR 8) or 32 (two passes, 4 KB per wave)
//   same tables (8 and 32 MB), same dependent chain (word 0 of every chunk read = part of the next index), same occupancies;
//   a combination whose staging does not fit 160 KB of LDS per CU at the asked occupancy is not run.
// Every cooperative run is checked against the per-lane kernel's output, word for word.
// What the figures are NOT: a forecast for wf_resume. Here every lane wants a DIFFERENT record; the 64 pixels of a wave there mostly
// hit a handful of objects, lanes with one address are one access already, and the cooperative form lost 0.3-0.4 ms per cfg4 frame
// (docs/LOG.md). CU-cycles are computed for 256 CUs at 2.4 GHz (MI355X), as in gather_rate.hip.
// Build / run on an MI355X:  hipcc --offload-arch=gfx950 -O3 coop_gather_rate.hip -o coop_gather_rate && ./coop_gather_rate
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %d (%s) at %d\n", (int)e, hipGetErrorString(e), __LINE__); return 1; } } while (0)

constexpr int kIters = 400;

// per lane: LOADS chunks [C0, C0 + LOADS) of one block
template <int LOADS, int C0>
__global__ __launch_bounds__(256) void chase(const uint4* __restrict__ table, uint32_t mask, int iters, uint32_t* __restrict__ out) {
    uint32_t idx = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
    uint32_t acc = 0;
    for (int it = 0; it < iters; ++it) {
        uint4 v[LOADS];
#pragma unroll
        for (int l = 0; l < LOADS; ++l) v[l] = table[(size_t)(idx & mask) * 8u + (uint32_t)(C0 + l)];
        uint32_t nx = 0;
#pragma unroll
        for (int l = 0; l < LOADS; ++l) { nx ^= v[l].x; acc += v[l].y ^ v[l].w; }
        idx = nx + (uint32_t)it;
    }
    out[blockIdx.x * 256u + threadIdx.x] = acc + idx;
}

// cooperative: LPR lanes per record, chunks [C0, C0 + LPR) fetched and [C0, C0 + CHUNKS) read back, STAGE lanes staged at a time
template <int CHUNKS, int C0, int LPR, int STAGE>
__global__ __launch_bounds__(256) void chase_coop(const uint4* __restrict__ table, uint32_t mask, int iters, uint32_t* __restrict__ out) {
    static_assert(CHUNKS <= LPR && C0 + LPR <= 8 && (LPR == 8 || LPR == 4) && (STAGE == 64 || STAGE == 32), "shape: the chunks fetched lie inside the record");
    constexpr int RPI = 64 / LPR;          // records per wave instruction
    constexpr int INSTR = STAGE / RPI;     // load instructions per pass
    constexpr int SW = 16 / LPR;           // staged records that share a swizzle
    __shared__ uint4 stage_all[4][STAGE * LPR];
    uint4* stage = stage_all[threadIdx.x >> 6];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t chunk = lane % LPR, sub = lane / LPR;
    uint32_t idx = (blockIdx.x * 256u + threadIdx.x) * 2654435761u;
    uint32_t acc = 0;
    for (int it = 0; it < iters; ++it) {
        uint4 v[CHUNKS];
#pragma unroll
        for (int base = 0; base < 64; base += STAGE) {
            uint4 got[INSTR];
#pragma unroll
            for (int j = 0; j < INSTR; ++j) {
                const uint32_t r = (uint32_t)(RPI * j) + sub;  // staged record = lane base + r
                const uint32_t want = (uint32_t)__shfl((int)idx, (int)(base + r), 64) & mask;
                got[j] = table[(size_t)want * 8u + (uint32_t)C0 + chunk];
            }
#pragma unroll
            for (int j = 0; j < INSTR; ++j) {
                const uint32_t r = (uint32_t)(RPI * j) + sub;
                stage[r * LPR + (chunk ^ ((r / SW) % LPR))] = got[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (STAGE == 64 || (lane >= (uint32_t)base && lane < (uint32_t)(base + STAGE))) {
                const uint32_t r = lane - (uint32_t)base;
#pragma unroll
                for (int k = 0; k < CHUNKS; ++k) v[k] = stage[r * LPR + ((uint32_t)k ^ ((r / SW) % LPR))];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        uint32_t nx = 0;
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k) { nx ^= v[k].x; acc += v[k].y ^ v[k].w; }
        idx = nx + (uint32_t)it;
    }
    out[blockIdx.x * 256u + threadIdx.x] = acc + idx;
}

struct Bench {
    const uint4* d_table;
    uint32_t* d_out;
    std::vector<uint32_t> ref, got;
};

template <typename K>
int time_kernel(K launch, int waves_per_simd, float& best) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    best = 1e30f;
    for (int rep = 0; rep < 3; ++rep) {
        CK(hipEventRecord(e0));
        launch(dim3(256 * waves_per_simd), dim3(256));  // 256 CUs x 4 SIMDs x waves / 4 waves per workgroup
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        CK(hipGetLastError());
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (ms < best) best = ms;
    }
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return 0;
}

void report(double table_mb, int w, int chunks, const char* form, float best, const char* check) {
    const double fetches = 256.0 * w * 256.0 * kIters;
    const double per_s = fetches / (best * 1e-3);
    const double cyc = 256.0 * 2.4e9 / per_s;  // CU cycles per lane-record
    printf("table %6.0f MB  waves/SIMD %d  chunks/record %d  %-34s  %7.3f ms  %7.1f G lane-records/s  %6.2f CU-cycles per lane-record  %s\n",
           table_mb, w, chunks, form, best, per_s / 1e9, cyc, check);
}

template <int LOADS, int C0>
int run_lane(Bench& b, uint32_t n_blocks, int w, double mb) {
    float best;
    if (time_kernel([&](dim3 g, dim3 t) { chase<LOADS, C0><<<g, t>>>(b.d_table, n_blocks - 1u, kIters, b.d_out); }, w, best)) return 1;
    b.ref.resize((size_t)256 * w * 256);
    CK(hipMemcpy(b.ref.data(), b.d_out, b.ref.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    report(mb, w, LOADS, "per lane (one 128-B block)", best, "");
    return 0;
}

template <int CHUNKS, int C0, int LPR, int STAGE>
int run_coop(Bench& b, uint32_t n_blocks, int w, double mb) {
    char form[64];
    snprintf(form, sizeof form, "cooperative %d lanes/record, stage %d", LPR, STAGE);
    const size_t lds_per_cu = (size_t)4 * w * STAGE * LPR * sizeof(uint4);
    if (lds_per_cu > 160u * 1024u) {
        printf("table %6.0f MB  waves/SIMD %d  chunks/record %d  %-34s  not run: %zu KB of LDS per CU\n", mb, w, CHUNKS, form, lds_per_cu / 1024);
        return 0;
    }
    CK(hipMemset(b.d_out, 0, (size_t)256 * w * 256 * sizeof(uint32_t)));
    float best;
    if (time_kernel([&](dim3 g, dim3 t) { chase_coop<CHUNKS, C0, LPR, STAGE><<<g, t>>>(b.d_table, n_blocks - 1u, kIters, b.d_out); }, w, best)) return 1;
    b.got.resize((size_t)256 * w * 256);
    CK(hipMemcpy(b.got.data(), b.d_out, b.got.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const bool same = b.got.size() == b.ref.size() && memcmp(b.got.data(), b.ref.data(), b.got.size() * sizeof(uint32_t)) == 0;
    report(mb, w, CHUNKS, form, best, same ? "= per lane" : "DIFFERS from per lane");
    return same ? 0 : 1;
}

int main() {
    const size_t max_blocks = (size_t)1 << 18;  // 32 MB
    std::vector<uint4> h(max_blocks * 8);
    uint64_t s = 88172645463325252ull;
    for (size_t i = 0; i < h.size(); ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        h[i] = make_uint4((uint32_t)(s >> 11), (uint32_t)s, 0u, (uint32_t)(s >> 40));
    }
    uint4* d_table;
    Bench b;
    CK(hipMalloc((void**)&d_table, h.size() * sizeof(uint4)));
    CK(hipMalloc((void**)&b.d_out, 256 * 8 * 256 * sizeof(uint32_t)));
    CK(hipMemcpy(d_table, h.data(), h.size() * sizeof(uint4), hipMemcpyHostToDevice));
    b.d_table = d_table;
    for (int pass = 0; pass < 2; ++pass) {  // everything twice: the spread between the two passes is the noise floor
        for (uint32_t lg : {16u, 18u}) {
            const uint32_t nb = 1u << lg;
            const double mb = nb * 128.0 / 1048576.0;
            for (int w : {4, 6, 8}) {
                if (run_lane<8, 0>(b, nb, w, mb)) return 1;
                if (run_coop<8, 0, 8, 64>(b, nb, w, mb)) return 1;
                if (run_coop<8, 0, 8, 32>(b, nb, w, mb)) return 1;
                if (run_lane<7, 0>(b, nb, w, mb)) return 1;
                if (run_coop<7, 0, 8, 64>(b, nb, w, mb)) return 1;
                if (run_coop<7, 0, 8, 32>(b, nb, w, mb)) return 1;
                if (run_lane<3, 4>(b, nb, w, mb)) return 1;
                if (run_coop<3, 4, 4, 64>(b, nb, w, mb)) return 1;
                if (run_coop<3, 4, 4, 32>(b, nb, w, mb)) return 1;
            }
        }
    }
    return 0;
}
