// Microbenchmark: where a stage of the forward roll-out spends its time at one wave per SIMD.  The stage of the kernel
// (mpcb_kernel.h, "forward roll-out") is: 9 per-lane LDS reads for the NEXT stage, a chain of 6 dependent v_fma_f64 whose
// multiplicands are scalar registers, 2 x v_readlane of the result, 2 more FMAs, a predicated LDS store, 4 x v_readlane.
// MODE 0 = all of it; 1 = without the LDS reads; 2 = without the readlanes (operands stay vector registers);
// 3 = only the eight FMAs; 4 = reads + FMAs, no readlanes, no store
#include <hip/hip_runtime.h>
#include <cstdio>

__device__ inline double rdlane(double v, int l) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}

template <int MODE>
__global__ __launch_bounds__(64) void k(double* out, long long* cyc, int stages) {
  __shared__ double fw[64 * 31];
  __shared__ double hist[8 * 65];
  const int lane = threadIdx.x;
  for (int i = lane; i < 64 * 31; i += 64) fw[i] = 1e-3 * ((i * 7) % 13) - 5e-3;
  __syncthreads();
  const int li = lane < 6 ? lane : 0;
  int fo[9];
  for (int r = 0; r < 9; ++r) fo[r] = (li * 5 + r * 3) % 31;
  double c[9], n9[9];
  for (int r = 0; r < 9; ++r) n9[r] = 0;
  for (int r = 0; r < 9; ++r) c[r] = fw[fo[r]];
  double v0 = 0.1, v1 = 0.2, v2 = 0.3, v3 = 0.4, v4 = 0.5, v5 = 0.6;
  long long t0 = __builtin_amdgcn_s_memtime();
#pragma clang loop unroll(disable)
  for (int s = 0; s < stages; ++s) {
    if (MODE == 0 || MODE == 4) {
      const double* q = fw + ((s + 1) & 63) * 31;
#pragma unroll
      for (int r = 0; r < 9; ++r) n9[r] = q[fo[r]];
      __builtin_amdgcn_sched_barrier(0);
    }
    if (MODE == 5 || MODE == 6 || MODE == 7) {
      const double* q = fw + ((s + 1) & 63) * 31;
      if (lane < (MODE == 5 ? 6 : MODE == 6 ? 16 : 32)) {
#pragma unroll
        for (int r = 0; r < 9; ++r) n9[r] = q[fo[r]];
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    double t = __builtin_fma(c[5], v5, __builtin_fma(c[4], v4, __builtin_fma(c[3], v3, __builtin_fma(c[2], v2, __builtin_fma(c[1], v1, __builtin_fma(c[0], v0, c[6]))))));
    double du0, du1;
    if (MODE == 0 || MODE == 1 || MODE >= 5) { du0 = rdlane(t, 4); du1 = rdlane(t, 5); } else { du0 = t; du1 = t * 0.5; }
    const double n = __builtin_fma(c[8], du1, __builtin_fma(c[7], du0, t));
    if (MODE == 0 || MODE == 1 || MODE >= 5) {
      if (lane < 6) hist[li * 65 + (s & 63)] = n;
      v0 = rdlane(n, 0); v1 = rdlane(n, 1); v2 = rdlane(n, 2); v3 = rdlane(n, 3);
    } else { v0 = n; v1 = n; v2 = n; v3 = n; }
    v4 = du0; v5 = du1;
    if (MODE == 0 || MODE >= 4) {
#pragma unroll
      for (int r = 0; r < 9; ++r) c[r] = n9[r];
    }
  }
  long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * 64 + lane] = v0 + v1 + v2 + v3 + v4 + v5 + hist[lane];
  if (lane == 0) cyc[blockIdx.x] = t1 - t0;
}
// The stage as the kernel has it now, records of 8 doubles read as four 16-byte reads from one address (row stride 50, as fw):
// QUAD = 0: the scalar form (lane i < 6 = row i, one chain, 12 v_readlane);
// QUAD = 1: the quad form (lane p of a quad = state row p, lanes p = 0, 1 also the gain rows as a second chain, eight 16-byte
//           reads, 14 v_mov_b32 DPP quad_perm instead of the readlanes);
// QUAD = 2: the row form (lane i < 6 of EVERY 16-lane row = row i, one chain as in the scalar form, the six numbers by
//           12 v_mov_b32 DPP row_newbcast: lane i of a row to the whole row);
// QUAD = 3: the row form with 6 v_mov_b64 DPP
template <int CTRL> __device__ inline double qperm(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  int lo = (int)b, hi = (int)(b >> 32);
  lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
// one v_mov_b64 DPP (64-bit DPP takes row_newbcast only); `old` is a dead value whose registers the result takes (every lane is
// written, so it is never seen): without it the compiler has to clear or copy a register pair first
template <int CTRL> __device__ inline double qperm64(double old, double v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xF, 0xF, false); }
#define CHAIN(c, c0) __builtin_fma(c[5], v5, __builtin_fma(c[4], v4, __builtin_fma(c[3], v3, __builtin_fma(c[2], v2, __builtin_fma(c[1], v1, __builtin_fma(c[0], v0, c0))))))
template <int QUAD>
__global__ __launch_bounds__(64) void kq(double* out, long long* cyc, int stages) {
  constexpr int FWS = 50, FWR = 8;
  __shared__ __attribute__((aligned(16))) double fw[64 * FWS];
  __shared__ double histm[8 * 65];
  const int lane = threadIdx.x;
  for (int i = lane; i < 64 * FWS; i += 64) fw[i] = 1e-3 * ((i * 7) % 13) - 5e-3;
  __syncthreads();
  int lq = lane; asm volatile("" : "+v"(lq));
  double* hist = histm + (lq < 6 ? lq : 6 + (lq & 1)) * 65;
  struct Rec { double c[6], c0, bx, g[6], g0, gx; };
  const int li = QUAD == 1 ? (lq & 3) : QUAD >= 2 ? ((lq & 15) < 6 ? (lq & 15) : 0) : (lq < 6 ? lq : 0);
  auto load = [&](int s, Rec& f) {
    const double* q = (const double*)__builtin_assume_aligned(fw + (s & 63) * FWS + li * FWR, 16);
#pragma unroll
    for (int r = 0; r < 6; ++r) f.c[r] = q[r];
    f.c0 = q[6]; f.bx = q[7];
    if (QUAD == 1) {
      const double* p = (const double*)__builtin_assume_aligned(fw + (s & 63) * FWS + (4 + (lq & 1)) * FWR, 16);
#pragma unroll
      for (int r = 0; r < 6; ++r) f.g[r] = p[r];
      f.g0 = p[6]; f.gx = p[7];
    }
  };
  double v0 = 0.1, v1 = 0.2, v2 = 0.3, v3 = 0.4, v4 = 0.5, v5 = 0.6;
  const bool gain_lane = (lq >> 1) == 2;
  auto stage = [&](int s, const Rec& f, Rec& nxt) {
    load(s + 1, nxt);
    __builtin_amdgcn_sched_barrier(0);
    const double t = CHAIN(f.c, f.c0);
    if (QUAD == 3) {
      const double du0 = qperm64<0x154>(v4, t), du1 = qperm64<0x155>(v5, t);
      const double n = __builtin_fma(f.bx, lq == 3 ? du1 : du0, t);
      hist[s & 63] = n;
      v0 = qperm64<0x150>(v0, n); v1 = qperm64<0x151>(v1, n); v2 = qperm64<0x152>(v2, n); v3 = qperm64<0x153>(v3, n); v4 = du0; v5 = du1;
    } else if (QUAD == 2) {
      const double du0 = qperm<0x154>(t), du1 = qperm<0x155>(t);
      const double n = __builtin_fma(f.bx, lq == 3 ? du1 : du0, t);
      hist[s & 63] = n;
      v0 = qperm<0x150>(n); v1 = qperm<0x151>(n); v2 = qperm<0x152>(n); v3 = qperm<0x153>(n); v4 = du0; v5 = du1;
    } else if (QUAD == 1) {
      const double tg = CHAIN(f.g, f.g0);
      const double du0 = qperm<0x00>(tg), du1 = qperm<0x55>(tg);
      const double n = __builtin_fma(f.bx, qperm<0x40>(tg), t);
      const double ng = __builtin_fma(f.gx, du0, tg);
      hist[s & 63] = gain_lane ? ng : n;
      v0 = qperm<0x00>(n); v1 = qperm<0x55>(n); v2 = qperm<0xAA>(n); v3 = qperm<0xFF>(n); v4 = du0; v5 = du1;
    } else {
      const double du0 = rdlane(t, 4), du1 = rdlane(t, 5);
      const double n = __builtin_fma(f.bx, lq == 3 ? du1 : du0, t);
      hist[s & 63] = n;
      v0 = rdlane(n, 0); v1 = rdlane(n, 1); v2 = rdlane(n, 2); v3 = rdlane(n, 3); v4 = du0; v5 = du1;
    }
  };
  Rec fA, fB;
  load(0, fA);
  long long t0 = __builtin_amdgcn_s_memtime();
#pragma clang loop unroll(disable)
  for (int s = 0; s + 1 < stages; s += 2) { stage(s, fA, fB); stage(s + 1, fB, fA); }
  long long t1 = __builtin_amdgcn_s_memtime();
  out[blockIdx.x * 64 + lane] = v0 + v1 + v2 + v3 + v4 + v5 + histm[lane];
  if (lane == 0) cyc[blockIdx.x] = t1 - t0;
}
template <int QUAD>
void runq(const char* what, int grid = 1024) {
  double* out; long long* cyc;
  (void)hipMalloc(&out, 1024 * 64 * 8); (void)hipMalloc(&cyc, 1024 * 8);
  const int stages = 3000;
  for (int rep = 0; rep < 2; ++rep) kq<QUAD><<<grid, 64>>>(out, cyc, stages);
  (void)hipDeviceSynchronize();
  long long h[1024]; (void)hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
  double s = 0; for (int i = 0; i < grid; ++i) s += h[i];
  printf("%-70s %.1f ticks per stage (grid %d)\n", what, s / grid / stages, grid);
  (void)hipFree(out); (void)hipFree(cyc);
}

template <int MODE>
void run(const char* what, int grid = 1024) {
  double* out; long long* cyc;
  (void)hipMalloc(&out, 1024 * 64 * 8); (void)hipMalloc(&cyc, 1024 * 8);
  const int stages = 3000;
  for (int rep = 0; rep < 2; ++rep) k<MODE><<<grid, 64>>>(out, cyc, stages);
  (void)hipDeviceSynchronize();
  long long h[1024]; (void)hipMemcpy(h, cyc, sizeof(h), hipMemcpyDeviceToHost);
  double s = 0; for (int i = 0; i < grid; ++i) s += h[i];
  printf("%-70s %.1f ticks per stage (grid %d)\n", what, s / grid / stages, grid);
  (void)hipFree(out); (void)hipFree(cyc);
}
int main() {
  run<0>("full stage (9 LDS reads, 8 FMAs, 12 readlanes, store)");
  run<1>("without the LDS reads");
  run<2>("without the readlanes and the store (vector operands)");
  run<3>("only the eight dependent FMAs");
  run<4>("LDS reads + FMAs, no readlanes");
  run<0>("full stage", 256);
  run<0>("full stage", 1);
  run<1>("without the LDS reads", 1);
  run<3>("only the eight dependent FMAs", 1);
  run<5>("full stage, LDS reads by lanes 0..5 only");
  run<6>("full stage, LDS reads by lanes 0..15 only");
  run<7>("full stage, LDS reads by lanes 0..31 only");
  runq<0>("kernel stage, scalar form (4 x 16-byte reads, 7 FMAs, 12 readlanes)");
  runq<1>("kernel stage, quad form (8 x 16-byte reads, 14 FMAs, 14 DPP moves)");
  runq<2>("kernel stage, row form (4 x 16-byte reads, 7 FMAs, 12 DPP moves)");
  runq<3>("kernel stage, row form, 64-bit DPP (4 x 16-byte reads, 7 FMAs, 6 DPP moves)");
  runq<0>("kernel stage, scalar form", 1);
  runq<1>("kernel stage, quad form", 1);
  runq<2>("kernel stage, row form", 1);
  runq<3>("kernel stage, row form, 64-bit DPP", 1);
  return 0;
}
