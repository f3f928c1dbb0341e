// D5b: the Winograd F(4x4, 3x3) transforms, shared by the three-call path (emp_conv.hip) and the one-kernel path
// (emp_wino4.hip).  Every operation is one fp32 rounding; the vector types differ only in how many channels a thread
// carries, so v1, v2 and v4 give the same bits per channel.
// B^T (Lavin & Gray), evaluated as:  r0 = (4 d0 - 5 d2) + d4;  r1 = (d3 + d4) - 4 (d1 + d2);
//   r2 = (d4 - d3) + 4 (d1 - d2);  r3 = (d4 - d2) + 2 (d3 - d1);  r4 = (d4 - d2) + 2 (d1 - d3);  r5 = (4 d1 - 5 d3) + d5
// A^T:  s0 = ((m0 + m1) + m2) + (m3 + m4);  s1 = (m1 - m2) + 2 (m3 - m4);  s2 = (m1 + m2) + 4 (m3 + m4);
//   s3 = ((m1 - m2) + 8 (m3 - m4)) + m5
#pragma once
#include <hip/hip_runtime.h>

struct v4 {
    float x, y, z, w;
};
__device__ __forceinline__ v4 operator+(v4 a, v4 b) { return {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y), __fadd_rn(a.z, b.z), __fadd_rn(a.w, b.w)}; }
__device__ __forceinline__ v4 operator-(v4 a, v4 b) { return {__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z), __fsub_rn(a.w, b.w)}; }
__device__ __forceinline__ v4 operator*(float k, v4 a) { return {__fmul_rn(k, a.x), __fmul_rn(k, a.y), __fmul_rn(k, a.z), __fmul_rn(k, a.w)}; }
__device__ __forceinline__ v4 ldv4(const float4 *p) { float4 t = *p; return {t.x, t.y, t.z, t.w}; }
__device__ __forceinline__ void stv4(float4 *p, v4 a) { *p = make_float4(a.x, a.y, a.z, a.w); }

struct v2 {
    float x, y;
};
__device__ __forceinline__ v2 operator+(v2 a, v2 b) { return {__fadd_rn(a.x, b.x), __fadd_rn(a.y, b.y)}; }
__device__ __forceinline__ v2 operator-(v2 a, v2 b) { return {__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y)}; }
__device__ __forceinline__ v2 operator*(float k, v2 a) { return {__fmul_rn(k, a.x), __fmul_rn(k, a.y)}; }

struct v1 {
    float x;
};
__device__ __forceinline__ v1 operator+(v1 a, v1 b) { return {__fadd_rn(a.x, b.x)}; }
__device__ __forceinline__ v1 operator-(v1 a, v1 b) { return {__fsub_rn(a.x, b.x)}; }
__device__ __forceinline__ v1 operator*(float k, v1 a) { return {__fmul_rn(k, a.x)}; }

template <class V>
__device__ __forceinline__ void wino4_bt(const V d[6], V r[6])
{
    r[0] = (4.f * d[0] - 5.f * d[2]) + d[4];
    r[1] = (d[3] + d[4]) - 4.f * (d[1] + d[2]);
    r[2] = (d[4] - d[3]) + 4.f * (d[1] - d[2]);
    r[3] = (d[4] - d[2]) + 2.f * (d[3] - d[1]);
    r[4] = (d[4] - d[2]) + 2.f * (d[1] - d[3]);
    r[5] = (4.f * d[1] - 5.f * d[3]) + d[5];
}

template <class V>
__device__ __forceinline__ void wino4_at(const V m[6], V s[4])
{
    s[0] = ((m[0] + m[1]) + m[2]) + (m[3] + m[4]);
    s[1] = (m[1] - m[2]) + 2.f * (m[3] - m[4]);
    s[2] = (m[1] + m[2]) + 4.f * (m[3] + m[4]);
    s[3] = ((m[1] - m[2]) + 8.f * (m[3] - m[4])) + m[5];
}
