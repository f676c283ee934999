// hermite6_pack.inc -- body i of the caller's state -> {pos, vel, acc_in or 0} in state12, as text; `zero`, when given, <- 0.  One text for
// hermite6_pack (hermite6_eval.hip) and hermite6_ensemble_pack (hermite6_ensemble.hip).  The includer has defined T, vec4, the arrays pos,
// vel, acc_in (may be null), zero (may be null) and state12, and the body's index i in them.
    const vec4 p = reinterpret_cast<const vec4*>(pos)[i], v = reinterpret_cast<const vec4*>(vel)[i];
    T          bx = 0, by = 0, bz = 0;
    if (acc_in) {
        const vec4 b = reinterpret_cast<const vec4*>(acc_in)[i];
        bx = b.x, by = b.y, bz = b.z;
    }
    vec4* const out = reinterpret_cast<vec4*>(state12) + 3 * static_cast<size_t>(i);
    out[0] = p;
    out[1] = vec4{v.x, v.y, v.z, 0};
    out[2] = vec4{bx, by, bz, 0};
    if (zero) reinterpret_cast<vec4*>(zero)[i] = vec4{0, 0, 0, 0};
