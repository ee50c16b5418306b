// tools/fz_check_gpu.hip -- the device build of fz.cuh / ecz.cuh against big integers: runs fz_mul, fz_sqr, fz_mul2 and the curve
// formulas (xyzzz_madd, xyzzz_add, xyzzz_dbl and the four-lane xyzzz_add_quad) on the GPU over operands prepared on the host and
// prints the cases in tools/fz_check.cpp's line format, so tools/fz_check.py verifies them (pass --device: the host-only line kinds
// are then not required).
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I mpc-jellyfish_amd/csrc tools/fz_check_gpu.hip -o fz_check_gpu
//     ./fz_check_gpu | python tools/fz_check.py --device
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <random>
#include <vector>
#include "ecz.cuh"
using namespace mzk;
using Z = BlsFqZ;
using F = Fz<Z>;
constexpr int N = Z::ZN;
constexpr int T = 16;                      // table of multiples of the generator

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct FieldCase { F x, y, u, v, mul, sqr, mul2; };
struct CurveCase { XYZZZ<Z> p, q; AffineZ<Z> a; int neg; XYZZZ<Z> madd, add, dbl, quad; };

__global__ void field_kernel(FieldCase* c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    c[i].mul = fz_mul<Z>(c[i].x, c[i].y);
    c[i].sqr = fz_sqr<Z>(c[i].x);
    c[i].mul2 = fz_mul2<Z>(c[i].x, c[i].y, c[i].u, c[i].v);
}
__global__ void curve_kernel(CurveCase* c, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    c[i].madd = xyzzz_madd<Z>(c[i].p, c[i].a, c[i].neg != 0);
    c[i].add = xyzzz_add<Z>(c[i].p, c[i].q);
    c[i].dbl = xyzzz_dbl<Z>(c[i].p);
}
__global__ void quad_kernel(CurveCase* c, int n) {                  // four lanes per case; n * 4 is a multiple of the block size
    const int t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 2, role = t & 3;
    if (i >= n) return;
    const F* pa = role == 0 ? &c[i].p.x : role == 1 ? &c[i].p.y : role == 2 ? &c[i].p.zz : &c[i].p.zzz;
    const F* pb = role == 0 ? &c[i].q.x : role == 1 ? &c[i].q.y : role == 2 ? &c[i].q.zz : &c[i].q.zzz;
    const F r = xyzzz_add_quad<Z>(*pa, *pb, role);
    F* out = role == 0 ? &c[i].quad.x : role == 1 ? &c[i].quad.y : role == 2 ? &c[i].quad.zz : &c[i].quad.zzz;
    *out = r;
}

static void put(const F& a) { for (int i = 0; i < N; i++) std::printf(" %d", a.l[i]); }
static void put_pt(const XYZZZ<Z>& p) { put(p.x); put(p.y); put(p.zz); put(p.zzz); }

int main() {
    std::mt19937_64 rng(99);
    auto rnd = [&](int64_t bound) {
        F r;
        for (int i = 0; i < N - 1; i++) r.l[i] = (int32_t)((int64_t)(rng() % (uint64_t)(2 * bound + 1)) - bound);
        r.l[N - 1] = (int32_t)(rng() % (1u << 22)) - (1 << 21);
        return r;
    };
    const int nf = 256;
    std::vector<FieldCase> fc(nf);
    for (int i = 0; i < nf; i++) {
        const int64_t b = i % 4 == 3 ? (1 << 29) + 2 : (1 << 29);
        fc[i].x = rnd(b); fc[i].y = rnd(b); fc[i].u = rnd(b); fc[i].v = rnd(1 << 29);
        if (i % 8 == 7)
            for (F* f : {&fc[i].x, &fc[i].y, &fc[i].u, &fc[i].v})
                for (int k = 0; k < N - 1; k++) f->l[k] = (rng() & 1) ? (1 << 29) : -(1 << 29);
    }
    // curve operands from the host build of the same header (tools/fz_check.cpp verifies that build)
    Fp<Z> gx, gy;
    for (int i = 0; i < Z::N; i++) { gx.l[i] = Z::GEN_X[i]; gy.l[i] = Z::GEN_Y[i]; }
    AffineZ<Z> g;
    g.x = fz_from_boundary<Z>(gx); g.y = fz_from_boundary<Z>(gy);
    XYZZZ<Z> mult[T];
    AffineZ<Z> tab[T];
    XYZZZ<Z> acc = XYZZZ<Z>::inf();
    for (int i = 0; i < T; i++) {
        acc = xyzzz_madd<Z>(acc, g, false);
        mult[i] = acc;
        const F zi = fz_inv<Z>(acc.zzz), zzi = fz_sqr<Z>(fz_mul<Z>(zi, acc.zz));
        tab[i].x = fz_mul<Z>(acc.x, zzi); tab[i].y = fz_mul<Z>(acc.y, zi);
    }
    std::vector<CurveCase> cc;
    for (int i = 0; i < T; i++)
        for (int j = 0; j < T; j++) {
            CurveCase c;
            c.p = (i + j) % 5 == 4 ? XYZZZ<Z>::from_affine(tab[i]) : mult[i];      // ZZ = 1 as a fresh bucket has it, or a real one
            c.q = j % 3 == 2 ? XYZZZ<Z>::from_affine(tab[j]) : mult[j];
            c.neg = (i * 7 + j) & 1;
            if (c.neg) c.q.y = fz_neg<Z>(c.q.y);                                   // i == j: P + Q doubles, or cancels
            c.a = tab[j];
            if (i == 3 && j == 5) c.p = XYZZZ<Z>::inf();
            if (i == 5 && j == 3) { c.q = XYZZZ<Z>::inf(); c.a.x = F::zero(); c.a.y = F::zero(); }
            cc.push_back(c);
        }
    const int nc = (int)cc.size();
    FieldCase* dfc; CurveCase* dcc;
    CHECK(hipMalloc(&dfc, nf * sizeof(FieldCase)));
    CHECK(hipMalloc(&dcc, nc * sizeof(CurveCase)));
    CHECK(hipMemcpy(dfc, fc.data(), nf * sizeof(FieldCase), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dcc, cc.data(), nc * sizeof(CurveCase), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(field_kernel, dim3((nf + 63) / 64), dim3(64), 0, nullptr, dfc, nf);
    hipLaunchKernelGGL(curve_kernel, dim3((nc + 63) / 64), dim3(64), 0, nullptr, dcc, nc);
    static_assert((T * T * 4) % 64 == 0, "whole quads and whole blocks");
    hipLaunchKernelGGL(quad_kernel, dim3(nc * 4 / 64), dim3(64), 0, nullptr, dcc, nc);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(fc.data(), dfc, nf * sizeof(FieldCase), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(cc.data(), dcc, nc * sizeof(CurveCase), hipMemcpyDeviceToHost));
    for (const FieldCase& c : fc) {
        std::printf("mul 1 %d", (int)fz_is_zero<Z>(c.mul)); put(c.x); put(c.y); put(c.mul); std::printf("\n");
        std::printf("sqr 1 %d", (int)fz_is_zero<Z>(c.sqr)); put(c.x); put(c.sqr); std::printf("\n");
        std::printf("mul2 1 %d", (int)fz_is_zero<Z>(c.mul2)); put(c.x); put(c.y); put(c.u); put(c.v); put(c.mul2); std::printf("\n");
    }
    for (const CurveCase& c : cc) {
        std::printf("madd %d", c.neg); put_pt(c.p); put(c.a.x); put(c.a.y); put_pt(c.madd); std::printf("\n");
        std::printf("add"); put_pt(c.p); put_pt(c.q); put_pt(c.add); std::printf("\n");
        std::printf("dbl"); put_pt(c.p); put_pt(c.dbl); std::printf("\n");
        std::printf("add"); put_pt(c.p); put_pt(c.q); put_pt(c.quad); std::printf("\n");
    }
    return 0;
}
