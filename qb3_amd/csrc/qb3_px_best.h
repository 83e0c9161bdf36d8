// qb3_amd/csrc/qb3_px_best.h -- what the lane-per-block decoders of the 8-bit common-factor modes share (k_dec_px_best.hip: the whole
// raster; qb3_win_best.h: the window kernels): the parser of a unit that starts with the signal.
#pragma once
#include "qb3_px.h"

namespace qb3dev {

// A unit that started with the signal, read from LDS at bit `pos` (just behind the signal): g = the sixteen mag-sign values
// (common factor: of the DIVIDED group, not yet multiplied).  Returns false on a malformed unit.
// kind: 0 common factor with its own factor (*cfv = cf - 2), 1 common factor with the band's factor in force, 2 index form
__device__ __forceinline__ bool best_slow_unit(uint32_t pos, uint32_t oldrung, uint8_t (&g)[16], uint32_t *kind, uint32_t *cfv, uint32_t *rung_out, uint32_t *end) {
    typedef uint8_t T;
    constexpr uint32_t UB = 3, UMASK = 7;
    ReaderT<LdsWords> rd;
    rd.init(lds_at(0), pos, ~0ull >> 8);
    bool sig2;
    bool ok = true;
    const uint32_t r = (oldrung + get_switch_noflag<UB>(rd, sig2)) & UMASK;
    *cfv = 0; *rung_out = r;
    if (r != UMASK) {           // common factor (QB3decode.h:629-679)
        *kind = 1;
        uint32_t cfrung = r;
        if (rd.get(1)) {
            const uint32_t own = rd.get(1);
            if (own) {
                cfrung = (r + get_switch_noflag<UB>(rd, sig2)) & UMASK;
                if (cfrung == r || cfrung == 0) ok = false;
            }
            const uint32_t vr = (cfrung - own) & UMASK;
            uint32_t v;
            if (vr == 0) v = rd.get(1);
            else { const T t = get_value<T>(rd, vr); v = (vr >= 3) ? unswap<T>(t, vr) : t; }    // factor values: rungs 1, 2 unswapped (QB3encode.h:144-150)
            *cfv = (v + (own << cfrung)) & 0xffu;
            *kind = 0;
        }
        if (r) get_group<T, true>(rd, r, g);
        else {
            const uint32_t bits = rd.get(16);
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) g[i] = (T)((bits >> i) & 1);
        }
    } else {                    // index form (QB3decode.h:680-715)
        *kind = 2;
        const uint32_t r2 = (oldrung + get_switch_noflag<UB>(rd, sig2)) & UMASK;
        *rung_out = r2;
        if (r2 == 0) ok = false;
        uint64_t ix = 0;        // 16 x 3 bit indices packed
        uint32_t maxidx = 0, ibits = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            rd.ensure(4);
            const uint32_t x = (uint32_t)rd.buf;
            uint32_t v, len;    // plain rung 2 code
            if (!(x & 1)) { v = (x & 3) >> 1; len = 2; }
            else if (!(x & 2)) { v = ((x >> 2) & 1) | 2; len = 3; }
            else { v = ((x >> 2) & 3) | 4; len = 4; }
            rd.skip(len);
            ibits += len;
            ix |= (uint64_t)v << (3 * i);
            maxidx = v > maxidx ? v : maxidx;
        }
        if (ibits > 52) ok = false;
        T tab[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            tab[i] = 0;
            if (i <= maxidx && ok) { const T t = get_value<T>(rd, r2 ? r2 : 1); tab[i] = (r2 >= 3) ? unswap<T>(t, r2) : t; }
        }
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t j = (uint32_t)(ix >> (3 * i)) & 7;
            T v = tab[0];
#pragma unroll
            for (uint32_t k = 1; k < 8; k++) v = (j == k) ? tab[k] : v;
            g[i] = v;
        }
    }
    *end = (uint32_t)rd.position();
    return ok;
}

}  // namespace qb3dev
