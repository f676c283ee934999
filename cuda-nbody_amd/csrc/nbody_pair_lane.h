// nbody_pair_lane.h -- what the forces kernels of the pairwise layout share besides nbody_lane.h (nbody_pair.hip's pair_forces and
// nbody_pair_lead.hip's pair_forces_jpacked): the rotation of a body j through the wave, lane 0's value as a scalar, and how the
// workspace planes are accessed.  Included inside each translation unit's own anonymous namespace, after nbody_lane.h.
#pragma once

// The workspace planes (reaction sums, i-side sums) are written once by the forces kernel and read once by pair_finish / pair_reduce.  With
// -DNB_PAIR_NONTEMPORAL (tools/build_pair_variant.sh; the A/B of round 6: profiles/round6_nontemporal_ab.txt) those accesses carry the
// non-temporal hint, so that the streaming planes do not evict the 4 MiB position array from each XCD's L2.  Without the flag: plain accesses.
#ifdef NB_PAIR_NONTEMPORAL
#define NB_WS_STORE(ptr, value) __builtin_nontemporal_store((value), (ptr))
#define NB_WS_LOAD(ptr) __builtin_nontemporal_load(ptr)
#else
#define NB_WS_STORE(ptr, value) (*(ptr) = (value))
#define NB_WS_LOAD(ptr) (*(ptr))
#endif

// ---- rotation of whatever belongs to the body j: one lane onward (lane l reads lane l-1; lane 0 reads lane 63) --------------
constexpr int kWaveRor1 = 0x13C;
// (The same rotation on the LDS crossbar -- ds_bpermute_b32, off the vector ALU -- was tried: 10.36 against 10.08 ms, same box.)
__device__ __forceinline__ int rotate_bits(int v) { return __builtin_amdgcn_update_dpp(v, v, kWaveRor1, 0xf, 0xf, false); }
__device__ __forceinline__ float rotate(float x) { return __builtin_bit_cast(float, rotate_bits(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ double rotate(double x) {
    const unsigned long long b  = __builtin_bit_cast(unsigned long long, x);
    const unsigned           l2 = static_cast<unsigned>(rotate_bits(static_cast<int>(b & 0xffffffffull)));
    const unsigned           h2 = static_cast<unsigned>(rotate_bits(static_cast<int>(b >> 32)));
    return __builtin_bit_cast(double, (static_cast<unsigned long long>(h2) << 32) | l2);
}
__device__ __forceinline__ v2f rotate(v2f x) { return v2f{rotate(x.x), rotate(x.y)}; }
// ... and an addition on the way: rotate(x) + t as ONE instruction, v_add_f32_dpp wave_ror:1.  (hipcc folds a lane move into the
// instruction that reads it only when the move says what a lane without a source gets -- bound_ctrl; a rotation has no such lane.)
__device__ __forceinline__ float rotate_add(float x, float t) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), kWaveRor1, 0xf, 0xf, true)) + t;
}

// lane 0's value, as a wave-uniform (scalar) value
__device__ __forceinline__ float first_lane(float x) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x))); }
__device__ __forceinline__ double first_lane(double x) {
    const unsigned long long b  = __builtin_bit_cast(unsigned long long, x);
    const unsigned           lo = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(b & 0xffffffffull)));
    const unsigned           hi = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(b >> 32)));
    return __builtin_bit_cast(double, (static_cast<unsigned long long>(hi) << 32) | lo);
}

__device__ __forceinline__ float  both_halves(v2f a) { return a.x + a.y; }
__device__ __forceinline__ double both_halves(double a) { return a; }
