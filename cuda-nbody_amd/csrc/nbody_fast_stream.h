// nbody_fast_stream.h -- the wave-stream layout of the one-sided FAST step, shared by nbody_fast.hip (integrate_bodies_fast) and
// ensemble_fast.hip (one such step per system of an ensemble): the helpers below, and nbody_fast_stream.inc, the kernel body itself.
// See nbody_fast.hip's header for the layout.  Included inside each translation unit's own anonymous namespace, after nbody_lane.h.
#pragma once

// The same for a body j held in SCALAR registers (every lane of the wave meets the same body): its coordinates enter the
// subtractions as scalar operands, broadcast to both halves of a packed pair by op_sel.  `mrel`: relative mass, a vector.
template <typename T, int R, bool UNIT>
__device__ __forceinline__ void interact_uniform(const typename Lane<T>::raw4 bj, const typename Lane<T>::vec mrel, const typename Lane<T>::vec (&px)[R], const typename Lane<T>::vec (&py)[R], const typename Lane<T>::vec (&pz)[R],
                                                 typename Lane<T>::vec (&ax)[R], typename Lane<T>::vec (&ay)[R], typename Lane<T>::vec (&az)[R], const typename Lane<T>::vec eps2, const typename Lane<T>::Consts& consts) {
    using L   = Lane<T>;
    using vec = typename L::vec;
    const vec bx = L::splat(bj.x), by = L::splat(bj.y), bz = L::splat(bj.z);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const vec dx = bx - px[r];
        const vec dy = by - py[r];
        const vec dz = bz - pz[r];
        vec       d2 = L::fma(dx, dx, eps2);
        d2           = L::fma(dy, dy, d2);
        d2           = L::fma(dz, dz, d2);
        const vec s  = L::template coupling_rel<UNIT>(mrel, d2, consts);
        ax[r]        = L::fma(dx, s, ax[r]);
        ay[r]        = L::fma(dy, s, ay[r]);
        az[r]        = L::fma(dz, s, az[r]);
    }
}

// The mass every sum of a j range is expressed in units of: the first body's, when the sums keep their range in units of it
// (usable_unit, nbody_lane.h: then an equal-mass range never multiplies by a mass inside the loop), otherwise 1.
template <typename T, typename Stream> __device__ __forceinline__ T reference_mass(const Shard<T>& s, Stream bodies) {
    if (s.j_count == 0) return T(1);
    const T m = bodies[s.j_begin].w;  // (a scalar load: the value is compared with scalar registers)
    return usable_unit(m) ? m : T(1);
}
