// The motion-field fit of ONE pair by a group of lanes, device side: the data movement around the rule of
// aof_field_step.hpp, written once for the kernels that fit -- k_field.hip (a batch's pairs) and k_bank_field.hip (the
// streams of a bank that ran a pair in the tick).  field_fit<GROUP, KEEP>: GROUP = 64, a wave per pair and four pairs per
// workgroup, for grids of at most 256 blocks (one quad of records per lane); GROUP = 256, a workgroup per pair, looping
// over the pair's quads, whatever their number.
//   * records as ALIGNED 16-byte loads, four records per lane and trip.  A pair's records start at any multiple of four
//     bytes (an odd grid puts pair 1 at + 4 mod 16), so up to three records in front of the first 16-byte boundary and up
//     to three behind the last whole quad are peeled: lanes 0..5 take one of them each, once.  Sub-directions four bytes at
//     a time beside their quad.
//   * per lane n, SX, SY, SU, SV in 32-bit registers (the bound: aof_field_step.hpp, "Ranges"), Q, A, C in 64 bits; wave
//     sums by cross-lane shuffles, the waves of a pair joined through LDS; lane 0 of the pair solves (field_solve) and
//     leaves a, b, tU, tV in LDS, so that every lane gates the second pass with the same bits.
//   * the second pass takes a lane's records from the registers the first pass loaded them into where a pair's quads fit
//     KEEP trips (every pair of the wave form; up to 5 120 records in the workgroup form: VGA's 4 661), and reads them again
//     otherwise.
// Integer sums do not depend on the order of addition, and the double operations are the rule's, one rounding each (built
// with contraction off): the record is the host's bit for bit.  Inputs are only read and nothing is stored: lane 0 of the
// group returns the pair's record, and what the other lanes return means nothing.
// Every lane of the group must call it (GROUP = 256: it holds workgroup barriers), with the same arguments.
#pragma once

#include "aof_device.hpp"
#include "aof_fastdiv.hpp"
#include "aof_field_step.hpp"

namespace aof {

namespace {

constexpr int kFieldThreads = 256;
constexpr int kFieldPart = 10;                      // n, SX, SY, SU, SV, Q, A, C, accepted, at_reach
constexpr uint32_t kFieldSkippedWord = 0xFFFF0000u; // a record nobody accepts: what a lane without a record holds

struct FieldLaneSums {
    int32_t n, SX, SY, SU, SV;
    int64_t Q, A, C;
};

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)(uint64_t)v, o, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)((uint64_t)v >> 32), o, 64);
        v += (int64_t)(((uint64_t)hi << 32) | lo);
    }
    return v;
}

// words / subdirs: the pair's own records ([nb], subdirs or nullptr); (px, py): its predictor.
template <int GROUP, int KEEP>
__device__ __forceinline__ aof_field field_fit(const FieldGeom &g, const FastDiv div_nx, const uint32_t *words, const uint8_t *subdirs,
                                               const int32_t px, const int32_t py)
{
    constexpr int kGroups = kFieldThreads / GROUP, kWaves = GROUP / 64;
    __shared__ int64_t s_part[kGroups][kWaves][kFieldPart];
    __shared__ double s_model[kGroups][4];
    __shared__ int32_t s_again[kGroups];
    const int grp = (int)threadIdx.x / GROUP, tid = (int)threadIdx.x % GROUP, wave = tid >> 6;
    // a wave-sized group needs no workgroup barrier: its LDS operations retire in program order
    auto sync = [] {
        if (GROUP == kFieldThreads) {
            __syncthreads();
        } else {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    };
    const int nb = g.nb, nx = g.nx;

    // the pair's records: `head` in front of the first 16-byte boundary, `quads` aligned quads, the rest behind them
    const int head = min(nb, (int)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(words) & 15u)) & 15u) >> 2));
    const int quads = (nb - head) >> 2, edge = nb - 4 * quads;   // edge = head + tail <= 6
    const int trips = (quads + GROUP - 1) / GROUP;
    const bool kept = trips <= KEEP;                             // (uniform) the second pass needs no load

    FieldLaneSums s;
    uint32_t accepted = 0, at_reach = 0;
    double ma = 0.0, mb = 0.0, mtU = 0.0, mtV = 0.0;
    auto clear = [&] { s.n = s.SX = s.SY = s.SU = s.SV = 0; s.Q = s.A = s.C = 0; };
    auto take = [&](uint32_t w, uint32_t sd, int32_t X, int32_t Y, bool gated) {
        const FieldRecord r = field_record(g, w, sd, px, py);
        if (!gated) { accepted += r.accepted; at_reach += r.at_reach; }
        bool in = field_member(g, r);
        if (gated && in) in = field_inlier(ma, mb, mtU, mtV, g.gate, X, Y, r.U, r.V);
        if (in) {
            s.n++; s.SX += X; s.SY += Y; s.SU += r.U; s.SV += r.V;
            s.Q += field_q(X, Y); s.A += field_a(X, Y, r.U, r.V); s.C += field_c(X, Y, r.U, r.V);
        }
    };

    // the peeled records: lane t < edge holds one, for both passes
    uint32_t ew = kFieldSkippedWord, esd = 8u;
    int32_t eX = 0, eY = 0;
    if (tid < edge) {
        const int k = tid < head ? tid : 4 * quads + tid;   // (= head + 4 quads + (tid - head) behind the quads)
        ew = words[k];
        if (subdirs) esd = subdirs[k];
        const int by = (int)fast_div((uint32_t)k, div_nx);
        eX = field_x(g, k - by * nx);
        eY = field_y(g, by);
    }

    uint4 rec[KEEP];
    uint32_t sdir[KEEP];
    auto load = [&](int t0) {   // every load of KEEP trips in flight before the first use
#pragma unroll
        for (int t = 0; t < KEEP; t++) {
            const int q = (t0 + t) * GROUP + tid;
            rec[t] = make_uint4(kFieldSkippedWord, kFieldSkippedWord, kFieldSkippedWord, kFieldSkippedWord);
            sdir[t] = 0x08080808u;
            if (q < quads) {
                rec[t] = *reinterpret_cast<const uint4 *>(words + head + 4 * q);
                if (subdirs) __builtin_memcpy(&sdir[t], subdirs + head + 4 * q, 4);
            }
        }
    };
    auto accumulate = [&](int t0, bool gated) {
#pragma unroll
        for (int t = 0; t < KEEP; t++) {
            const int q = (t0 + t) * GROUP + tid;
            if (q < quads) {
                const uint32_t k0 = (uint32_t)(head + 4 * q);
                int by = (int)fast_div(k0, div_nx), bx = (int)k0 - by * nx;
                // a real loop over the quad's records, which rotate through w.x (unrolled, the twenty copies of the rule
                // that five trips make need more than the 128 registers of four waves per SIMD)
                uint4 w = rec[t];
                uint32_t sd = sdir[t];
#pragma nounroll
                for (int j = 0; j < 4; j++) {
                    take(w.x, sd & 0xFFu, field_x(g, bx), field_y(g, by), gated);
                    w.x = w.y; w.y = w.z; w.z = w.w; sd >>= 8;
                    if (++bx == nx) { bx = 0; by++; }
                }
            }
        }
    };
    auto sweep = [&](bool gated) {
        clear();
        for (int t0 = 0; t0 < trips; t0 += KEEP) {   // (uniform)
            if (!(kept && gated)) load(t0);
            accumulate(t0, gated);
        }
        take(ew, esd, eX, eY, gated);
        // wave sums by shuffles, the pair's waves side by side in LDS
        const int32_t n = (int32_t)wave_sum_u32((uint32_t)s.n), SX = (int32_t)wave_sum_u32((uint32_t)s.SX);
        const int32_t SY = (int32_t)wave_sum_u32((uint32_t)s.SY), SU = (int32_t)wave_sum_u32((uint32_t)s.SU);
        const int32_t SV = (int32_t)wave_sum_u32((uint32_t)s.SV);
        const int64_t Q = wave_sum_i64(s.Q), A = wave_sum_i64(s.A), C = wave_sum_i64(s.C);
        const uint32_t acc = wave_sum_u32(accepted), rch = wave_sum_u32(at_reach);
        if ((tid & 63) == 0) {
            int64_t *part = s_part[grp][wave];
            part[0] = n; part[1] = SX; part[2] = SY; part[3] = SU; part[4] = SV;
            part[5] = Q; part[6] = A; part[7] = C; part[8] = acc; part[9] = rch;
        }
        sync();
    };
    auto total = [&](int i) {
        int64_t v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) v += s_part[grp][w][i];
        return v;
    };
    auto sums = [&] {
        FieldSums t;
        t.n = total(0); t.SX = total(1); t.SY = total(2); t.SU = total(3); t.SV = total(4);
        t.Q = total(5); t.A = total(6); t.C = total(7);
        return t;
    };

    sweep(false);
    aof_field f = field_publish(0u, 0u, 0u, nullptr, 0u, false);
    FieldModel m1;
    uint32_t n_accepted = 0, n_reach = 0, n_fitted = 0;
    if (tid == 0) {
        const FieldSums s1 = sums();
        n_accepted = (uint32_t)total(8);
        n_reach = (uint32_t)total(9);
        n_fitted = (uint32_t)s1.n;
        m1 = field_solve(s1, g.min_blocks);
        const bool again = m1.fits && g.passes == 2;
        s_model[grp][0] = m1.a; s_model[grp][1] = m1.b; s_model[grp][2] = m1.tU; s_model[grp][3] = m1.tV;
        s_again[grp] = again;
        if (!again) f = field_publish(n_accepted, n_reach, n_fitted, m1.fits ? &m1 : nullptr, n_fitted, false);
    }
    sync();
    if (!s_again[grp]) return f;   // (uniform in the group)
    ma = s_model[grp][0]; mb = s_model[grp][1]; mtU = s_model[grp][2]; mtV = s_model[grp][3];
    sweep(true);
    if (tid == 0) {
        const FieldSums s2 = sums();
        const FieldModel m2 = field_solve(s2, g.min_blocks);
        f = m2.fits ? field_publish(n_accepted, n_reach, n_fitted, &m2, (uint32_t)s2.n, true)
                    : field_publish(n_accepted, n_reach, n_fitted, &m1, n_fitted, false);
    }
    return f;
}

}  // namespace

}  // namespace aof
