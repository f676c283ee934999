// nbody_pair_lead.hip -- the forces kernel of the pairwise layout for ONE geometry, the headline's: fp32, sixteen bodies i per lane,
// eight waves, one workgroup per block, the whole tournament in one launch (launch_pair of nbody_pair.hip decides: pair_lead_takes).
// gfx950 (CDNA4) only.  Same PairArgs, grid, LDS size, workspace layout and pair_finish as pair_forces<float, 8, 8>; what differs is
// what a packed pair holds.
//
// pair_forces packs two bodies I into a register pair and meets one body j per step: the body j is three registers, but each of its
// three reaction sums is a PAIR (one half per body i of the pair, folded when the sum is stored) -- nine registers rotate per step
// for one body j, and a step is 8 x (14 v_pk_* + 2 v_rsq_f32) + 9 moves = 137 vector instructions for 16 pairs.
// pair_forces_jpacked packs two bodies J: a tile is 128 bodies, lane l holds bodies first + l and first + 64 + l as the two halves of
// jx, jy, jz, and each reaction sum is again a pair -- but now one half per body j, nothing to fold.  A body i enters a packed
// instruction as the broadcast of its half of a position pair (op_sel), and owns a packed pair per acceleration component whose halves
// are partial sums over the two bodies j (added once, at the end).  Twelve registers rotate for TWO bodies j: a step is
// 16 x (14 v_pk_* + 2 v_rsq_f32) + 12 moves = 268 vector instructions for 32 pairs, 8.375 per pair against 8.5625.
// A block pair is 8 units of 128 bodies j; with eight waves and one workgroup per block every wave takes exactly one unit of every
// block pair: no tail, no quarters (PairArgs::deal is not read).
#include "nbody_pair_lead.h"

namespace nb {
namespace {

#include "nbody_lane.h"
#include "nbody_pair_lane.h"

#ifndef NB_PAIR_LEAD_UNR
#define NB_PAIR_LEAD_UNR 1  // steps per trip of the rotation loop (a step is 268 vector instructions: two steps of pair_forces)
#endif
#ifndef NB_PAIR_LEAD_IB
#define NB_PAIR_LEAD_IB 4   // bodies i per stage block.  (UNR 2 or IB 2 leave register copies inside the one-species loop: 11 per trip)
#endif

template <int S> __global__ __launch_bounds__(64 * S) __attribute__((amdgpu_waves_per_eu(2, 2))) void pair_forces_jpacked(PairArgs<float> s) {
    using LT            = Lane<float>;
    using T             = float;
    using vec           = v2f;
    constexpr int I     = 16;        // bodies i per lane
    constexpr int P     = I / 2;     // ... their positions as register pairs
    constexpr int BLOCK = 64 * I;    // bodies per block
    constexpr int TB    = I / 2;     // 128-body tiles per block
    constexpr int UNR   = NB_PAIR_LEAD_UNR;  // steps per trip of the rotation loop

    extern __shared__ __attribute__((aligned(32))) unsigned char smem_raw[];

    const float4* __restrict__ old_pos = reinterpret_cast<const float4*>(s.old_pos);
    const int      tid  = threadIdx.x;
    const int      wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int      lane = tid & 63;
    const unsigned a    = blockIdx.x;  // the block whose bodies i this workgroup holds

    // bodies i of this lane: block_base + k*64 + lane (coalesced across the wave); a body beyond the range sits on its last body with mass 0
    const unsigned block_base = s.i_begin + a * BLOCK;
    const unsigned i_end      = s.i_begin + s.i_count;
    vec            px[P], py[P], pz[P];  // body i = k: half k % 2 of pair k / 2
    vec            ax[I], ay[I], az[I];  // body i = k: the halves are the partial sums over the two bodies j of a lane
    // Is the block ONE species -- every body i real and of the same mass m_block?  (Wave-uniform answer: each wave holds the whole block.)
    const T        m_block    = old_pos[block_base < i_end ? block_base : i_end - 1].w;  // (uniform address)
    const unsigned block_bits = __builtin_bit_cast(unsigned, m_block);
    bool           same       = true;
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const unsigned i = block_base + k * 64 + lane;
        const float4   p = old_pos[i < i_end ? i : i_end - 1];
        LT::set(px[k / 2], k % 2, p.x);
        LT::set(py[k / 2], k % 2, p.y);
        LT::set(pz[k / 2], k % 2, p.z);
        same = same && i < i_end && __builtin_bit_cast(unsigned, p.w) == block_bits;
    }
    const bool block_uniform = __builtin_amdgcn_ballot_w64(!same) == 0 && usable_scale(m_block);
#pragma unroll
    for (int k = 0; k < I; ++k) ax[k] = ay[k] = az[k] = LT::splat(0);
    vec eps2 = LT::splat(s.eps2);
    LT::keep_in_vgpr(eps2);
    const LT::Consts consts = LT::make_consts();

    // ---- LDS: [S][3*I][64] second-level sums -- later the fold buffer -- then the progress words (pair_forces' layout) ---------
    constexpr size_t kSumBytes = static_cast<size_t>(S) * 3 * I * 64 * sizeof(T);
    T* const         sums      = reinterpret_cast<T*>(smem_raw);
    unsigned* const  balance   = reinterpret_cast<unsigned*>(smem_raw + kSumBytes);
    unsigned* const  simd_count = balance;                                            // [4] waves of this workgroup per SIMD
    volatile unsigned* progress = reinterpret_cast<volatile unsigned*>(balance + 4);  // [4][8] units done, by SIMD and slot
    if (tid < 36) balance[tid] = tid < 4 ? 0u : 0xffffffffu;
    __syncthreads();
    // SIMD-mate balancing as in pair_forces: a wave level with the slowest wave of its SIMD runs at priority 3, one that is ahead at 0
    const unsigned simd = static_cast<unsigned>(__builtin_amdgcn_s_getreg((1 << 11) | (4 << 6) | 4));  // HW_REG_HW_ID[5:4] = SIMD_ID
    unsigned       slot = 0;
    if (lane == 0) slot = atomicAdd(&simd_count[simd], 1u);
    slot = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(slot))) & 7u;
    volatile unsigned* const mine = progress + simd * 8;
    unsigned                 done = 0;
    if (lane == 0) mine[slot] = 0;

    // A register sum collects at most kFlush tiles (1 024 bodies j, 512 per half), then joins the lane's second-level sum in LDS.  The
    // second level holds ONE word per body i and component (a word per half would take 192 KiB for eight waves): a flush adds the halves.
    constexpr unsigned kFlush = 8;
    T* const           second = sums + static_cast<size_t>(wave) * (3 * I * 64) + lane;
#pragma unroll
    for (int q = 0; q < 3 * I; ++q) second[q * 64] = 0;
    // The register sums are kept in units of `unit`, the mass of the species whose tiles the wave is working through (pair_forces)
    T unit = T(1);
    auto flush = [&](vec (&ax)[I], vec (&ay)[I], vec (&az)[I]) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            second[(0 * I + k) * 64] = __builtin_fmaf(both_halves(ax[k]), unit, second[(0 * I + k) * 64]);
            second[(1 * I + k) * 64] = __builtin_fmaf(both_halves(ay[k]), unit, second[(1 * I + k) * 64]);
            second[(2 * I + k) * 64] = __builtin_fmaf(both_halves(az[k]), unit, second[(2 * I + k) * 64]);
        }
#pragma unroll
        for (int k = 0; k < I; ++k) ax[k] = ay[k] = az[k] = LT::splat(0);
    };
    auto change_unit = [&](T to) {  // (wave-uniform)
        const vec ratio = LT::splat(unit / to);
#pragma unroll
        for (int k = 0; k < I; ++k) ax[k] = ax[k] * ratio, ay[k] = ay[k] * ratio, az[k] = az[k] * ratio;
        unit = to;
    };

    // ---- the units of this wave: unit u = tile u % TB of block a + u / TB; wave w takes u = w, w + S, ... -----------------------
    const unsigned NB      = s.blocks;
    const unsigned Q       = NB / 2;
    const bool     even    = (NB & 1u) == 0;
    const unsigned j_end   = s.j_begin + s.j_count;
    const unsigned n_units = (Q + 1) * TB;
    const unsigned n_items = static_cast<unsigned>(wave) < n_units ? (n_units - static_cast<unsigned>(wave) + S - 1) / S : 0;
    auto item_unit = [&](unsigned it) { return static_cast<unsigned>(wave) + it * S; };
    auto tile_first = [&](unsigned u) {
        unsigned jb = a + u / TB;
        if (jb >= NB) jb -= NB;
        return s.j_begin + jb * BLOCK + (u % TB) * 128;
    };
    struct Tile {
        float4 lo, hi;  // bodies first + lane and first + 64 + lane, as loaded: a body beyond the range is the last body (its mass is dropped when the tile is taken up)
    };
    auto load_tile = [&](unsigned u) {
        const unsigned j = tile_first(u) + static_cast<unsigned>(lane);
        return Tile{old_pos[j < j_end ? j : j_end - 1], old_pos[j + 64 < j_end ? j + 64 : j_end - 1]};
    };

    struct Reaction {
        float x0, x1, y0, y1, z0, z1;  // the sums of the lane's two bodies j (0: first + lane, 1: first + 64 + lane): six plain registers
    };
    // one rotation step: the lane's sixteen bodies i, one after the other, against the two bodies j it holds right now; then the
    // bodies j and their sums move on.  Written stage by stage over IB bodies i: IB independent chains.
    // MASSES: the general loop -- m_j / unit travels with the bodies j and multiplies the i side, the masses of the bodies i
    // multiply the reaction side; without it block and tile are one species each and nothing is multiplied by a mass.
    auto step = [&]<bool MASSES>(vec (&ax)[I], vec (&ay)[I], vec (&az)[I], vec (&px)[P], vec (&py)[P], vec (&pz)[P], vec& jx, vec& jy, vec& jz, vec& jm, Reaction& re, vec (&mi)[P]) {
        constexpr int IB = NB_PAIR_LEAD_IB;
        // (a body i is read as one HALF of its pair, op_sel on the packed instruction; left to itself hipcc forms the 24 broadcasts as
        // register pairs of their own ahead of the loop -- 48 registers more, and spills.  An empty statement per pair keeps them out.)
#pragma unroll
        for (int p = 0; p < P; ++p) {
            LT::keep_in_vgpr(px[p]), LT::keep_in_vgpr(py[p]), LT::keep_in_vgpr(pz[p]);
            if constexpr (MASSES) LT::keep_in_vgpr(mi[p]);
        }
        vec tx, ty, tz;  // the step's own reaction sums: sixteen terms, then one addition into the sums that travel
#pragma unroll
        for (int h = 0; h < I; h += IB) {
            vec dx[IB], dy[IB], dz[IB], w[IB];
#pragma unroll
            for (int r = 0; r < IB; ++r) {
                const int k = h + r;
                dx[r] = jx - LT::splat(LT::get(px[k / 2], k % 2)), dy[r] = jy - LT::splat(LT::get(py[k / 2], k % 2)), dz[r] = jz - LT::splat(LT::get(pz[k / 2], k % 2));
            }
#pragma unroll
            for (int r = 0; r < IB; ++r) w[r] = LT::fma(dx[r], dx[r], eps2);
#pragma unroll
            for (int r = 0; r < IB; ++r) w[r] = LT::fma(dy[r], dy[r], w[r]);
#pragma unroll
            for (int r = 0; r < IB; ++r) w[r] = LT::fma(dz[r], dz[r], w[r]);
#pragma unroll
            for (int r = 0; r < IB; ++r) w[r] = LT::coupling_rel<true>(eps2, w[r], consts);  // d2^(-3/2)
#pragma unroll
            for (int r = 0; r < IB; ++r) {
                const int k  = h + r;
                vec       wi = w[r], wj = w[r];
                if constexpr (MASSES) wi = jm * w[r], wj = LT::splat(LT::get(mi[k / 2], k % 2)) * w[r];
                ax[k] = LT::fma(dx[r], wi, ax[k]), ay[k] = LT::fma(dy[r], wi, ay[k]), az[k] = LT::fma(dz[r], wi, az[k]);
                if (k == 0) tx = dx[r] * wj, ty = dy[r] * wj, tz = dz[r] * wj;
                else tx = LT::fma(dx[r], wj, tx), ty = LT::fma(dy[r], wj, ty), tz = LT::fma(dz[r], wj, tz);
            }
        }
        // the bodies j and everything that belongs to them move on by one lane
        jx = rotate(jx), jy = rotate(jy), jz = rotate(jz);
        if constexpr (MASSES) jm = rotate(jm);
        re.x0 = rotate_add(re.x0, tx.x), re.x1 = rotate_add(re.x1, tx.y);
        re.y0 = rotate_add(re.y0, ty.x), re.y1 = rotate_add(re.y1, ty.y);
        re.z0 = rotate_add(re.z0, tz.x), re.z1 = rotate_add(re.z1, tz.y);
    };
    auto rotation_steps = [&]<bool MASSES>(vec (&ax)[I], vec (&ay)[I], vec (&az)[I], vec (&px)[P], vec (&py)[P], vec (&pz)[P], vec& jx, vec& jy, vec& jz, vec& jm, Reaction& re, vec (&mi)[P]) {  // a unit: 64 steps
#pragma unroll 1
        for (int it = 0; it < 64 / UNR; ++it) {
#pragma unroll
            for (int v = 0; v < UNR; ++v) step.template operator()<MASSES>(ax, ay, az, px, py, pz, jx, jy, jz, jm, re, mi);
        }
    };

    Tile cur = n_items > 0 ? load_tile(item_unit(0)) : Tile{};
    for (unsigned item = 0; item < n_items; ++item) {
        const unsigned u    = item_unit(item);
        const Tile     next = (item + 1) < n_items ? load_tile(item_unit(item + 1)) : cur;  // in flight across the steps below
        {
            unsigned least = done;
#pragma unroll
            for (int q = 0; q < 8; ++q) least = min(least, mine[q]);  // unsynchronised reads: a stale value only delays a priority change
            if (static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(least))) >= done) {
                __builtin_amdgcn_s_setprio(3);
            } else {
                __builtin_amdgcn_s_setprio(0);
            }
        }
        const unsigned q     = u / TB;  // the block offset
        const unsigned j     = tile_first(u) + static_cast<unsigned>(lane);  // the lane's bodies j: j and j + 64
        if (j >= j_end) cur.lo.w = 0;
        if (j + 64 >= j_end) cur.hi.w = 0;
        // Is the tile ONE species -- all 128 bodies j real and of one usable mass?  Then, in a block of one species, no mass is multiplied
        // in the loop: the wave's i-side sums are in units of the tile's mass, the block's mass multiplies the reaction sums when they are stored.
        const T    m_tile      = first_lane(cur.lo.w);
        const bool one_species = block_uniform && usable_unit(m_tile) &&
                                 __builtin_amdgcn_ballot_w64(!(j + 64 < j_end && __builtin_bit_cast(unsigned, cur.lo.w) == __builtin_bit_cast(unsigned, m_tile) &&
                                                               __builtin_bit_cast(unsigned, cur.hi.w) == __builtin_bit_cast(unsigned, m_tile))) == 0;
        vec jx = vec{cur.lo.x, cur.hi.x}, jy = vec{cur.lo.y, cur.hi.y}, jz = vec{cur.lo.z, cur.hi.z}, jm = LT::splat(0);
        Reaction re{};
        T   scale = T(1);  // what the reaction sums are still to be multiplied by
        if (one_species) {
            if (__builtin_bit_cast(unsigned, m_tile) != __builtin_bit_cast(unsigned, unit)) change_unit(m_tile);
            scale = m_block;
            vec none[P] = {};  // (this loop never reads the masses of the bodies i)
            rotation_steps.template operator()<false>(ax, ay, az, px, py, pz, jx, jy, jz, jm, re, none);
        } else {
            jm = vec{cur.lo.w, cur.hi.w} / LT::splat(unit);  // m_j / unit travels with the body j
            vec mi[P];  // the masses of the bodies i: only this path holds them, and only while it runs
#pragma unroll
            for (int k = 0; k < I; ++k) {
                const unsigned i = block_base + k * 64 + lane;
                LT::set(mi[k / 2], k % 2, i < i_end ? old_pos[i].w : T(0));
            }
            // This path works on copies of the positions and on sums of its own, flushed before and after.  Why: a step re-declares
            // the position pairs it reads (keep_in_vgpr, below in `step`), so two loops that both did that to px/py/pz and both added
            // to ax/ay/az would meet in 72 merged values after the branch, and the register allocator then pays for the general
            // loop's higher pressure on the ONE-SPECIES path: 78 scratch accesses per tile there (measured in the listing), none so.
            vec gx[P], gy[P], gz[P];
#pragma unroll
            for (int p = 0; p < P; ++p) gx[p] = px[p], gy[p] = py[p], gz[p] = pz[p];
            flush(ax, ay, az);
            vec bx[I], by[I], bz[I];
#pragma unroll
            for (int k = 0; k < I; ++k) bx[k] = by[k] = bz[k] = LT::splat(0);
            rotation_steps.template operator()<true>(bx, by, bz, gx, gy, gz, jx, jy, jz, jm, re, mi);
            flush(bx, by, bz);
        }
        // The travelling sums stay one lane BEHIND their bodies j, so that a step's own sums join them in the instruction that moves
        // them on (re(l) = re(l - 1) + t(l): the addition carries the lane move).  64 steps on the bodies j are home; one move more and so are the sums.
        re.x0 = rotate(re.x0), re.x1 = rotate(re.x1), re.y0 = rotate(re.y0), re.y1 = rotate(re.y1), re.z0 = rotate(re.z0), re.z1 = rotate(re.z1);
        // 64 steps on: every sum is back in the lane of its bodies j.  Keep the reaction only when the partner does not list the pair too.
        const bool symmetric = q != 0 && !(even && q == Q);
        if (symmetric) {
            T* const out = s.react + static_cast<size_t>(q - 1) * 3 * s.react_plane + (j - s.react_origin);
            if (j < j_end) {
                NB_WS_STORE(out, re.x0 * scale);
                NB_WS_STORE(out + static_cast<size_t>(s.react_plane), re.y0 * scale);
                NB_WS_STORE(out + 2 * static_cast<size_t>(s.react_plane), re.z0 * scale);
            }
            if (j + 64 < j_end) {
                NB_WS_STORE(out + 64, re.x1 * scale);
                NB_WS_STORE(out + static_cast<size_t>(s.react_plane) + 64, re.y1 * scale);
                NB_WS_STORE(out + 2 * static_cast<size_t>(s.react_plane) + 64, re.z1 * scale);
            }
        }
        cur = next;
        ++done;
        if (done % kFlush == 0) flush(ax, ay, az);
        if (lane == 0) mine[slot] = done;
    }
    if (lane == 0) mine[slot] = 0xffffffffu;  // finished: never the one the others defer to
    __builtin_amdgcn_s_setprio(0);

    // the two halves of every sum, once; absolute units; the second-level sums
    T fx[I], fy[I], fz[I];
#pragma unroll
    for (int k = 0; k < I; ++k) {
        fx[k] = second[(0 * I + k) * 64] + both_halves(ax[k]) * unit;
        fy[k] = second[(1 * I + k) * 64] + both_halves(ay[k]) * unit;
        fz[k] = second[(2 * I + k) * 64] + both_halves(az[k]) * unit;
    }

    // fold the S partial sums (waves 1..S-1 -> wave 0) through LDS, fixed order; the second-level sums are done with
    __syncthreads();
    T* const red = sums;  // [(S-1)][3][I][64]
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            red[(((wave - 1) * 3 + 0) * I + k) * 64 + lane] = fx[k];
            red[(((wave - 1) * 3 + 1) * I + k) * 64 + lane] = fy[k];
            red[(((wave - 1) * 3 + 2) * I + k) * 64 + lane] = fz[k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
#pragma unroll 1
    for (int w = 1; w < S; ++w) {
#pragma unroll
        for (int k = 0; k < I; ++k) {
            fx[k] += red[(((w - 1) * 3 + 0) * I + k) * 64 + lane];
            fy[k] += red[(((w - 1) * 3 + 1) * I + k) * 64 + lane];
            fz[k] += red[(((w - 1) * 3 + 2) * I + k) * 64 + lane];
        }
    }
    T* const self = s.self + static_cast<size_t>(s.self_first) * 3 * s.self_plane;
#pragma unroll
    for (int k = 0; k < I; ++k) {
        const unsigned i = block_base + k * 64 + lane;
        if (i >= i_end) continue;
        const size_t at = i - s.self_origin;
        NB_WS_STORE(self + at, fx[k]);
        NB_WS_STORE(self + static_cast<size_t>(s.self_plane) + at, fy[k]);
        NB_WS_STORE(self + 2 * static_cast<size_t>(s.self_plane) + at, fz[k]);
    }
}

}  // namespace

bool pair_lead_takes(const PairArgs<float>& a, const PairGeom& g) {
    size_t bytes = 0;
    return g.vectors_per_lane == 8 && g.waves == 8 && g.splits == 1 && a.diag != 0 && a.unit_begin == 0 && a.unit_count == 0 && a.i_count != 0 &&
           pair_clock_words(&bytes) == nullptr &&  // (lent words ask for pair_forces_clocked)
           pair_probe_event() == nullptr;           // (a probe event times pair_forces: the figure that goes with the clocked kernel's cycles)
}

hipError_t launch_pair_lead(const PairArgs<float>& args, hipStream_t stream, bool prepare_only) {
    constexpr int  S     = 8;
    PairArgs<float> a    = args;
    a.blocks             = (a.i_count + 1023u) / 1024u;
    a.splits             = 1;
    const unsigned lds_bytes = pair_lds_bytes(8, 2, S, sizeof(float), 0);  // (pair_forces<float, 8, 8> without quarters: 98 560 bytes)
    if (const auto err = allow_large_lds<&pair_forces_jpacked<S>>(); err != hipSuccess) return err;
    if (prepare_only) return hipSuccess;
    (void)hipGetLastError();  // a launch reports ITS OWN error: the call returns, and clears, the thread's last error whatever left it
    hipLaunchKernelGGL((pair_forces_jpacked<S>), dim3(a.blocks), dim3(64 * S), lds_bytes, stream, a);
    return hipGetLastError();
}

}  // namespace nb
