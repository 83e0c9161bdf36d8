// qb3_amd/csrc/probe_readers.hip -- libqb3probe.so: TEST INSTRUMENT ONLY.  Neither libQB3.so, bench.py nor the tools link
// or load it.  It instantiates the product's own bit readers (qb3_kernels.h, qb3_wide.h) -- nothing is restated here -- in
// plain kernels over caller-sized buffers, so that tests/test_bit_readers.py can compare every value they read with the
// code rule (tests/qb3_spec.py), over global memory and out of LDS, on a clean device and right after probe_dirty.
//
// Every kernel is bounded by what the caller says its buffers hold: a lane whose range does not fit is skipped and flagged,
// a reader reads zeros past its end (ReaderT::load), so a wrongly read value comes out as a wrong number, never as an address.
#include "qb3_kernels.h"
#include "qb3_wide.h"

using namespace qb3dev;

namespace {

constexpr uint32_t PROBE_LDS_DW = 8192;                 // stream words a workgroup stages (32 KiB), WIDE_PAD_DW zero words behind
constexpr uint32_t PROBE_TOO_BIG = 0xffffffffu;          // a lane's (workgroup's) range did not fit the staging
constexpr int DIRTY_REGS = 224;                          // VGPRs a lane of probe_dirty keeps live

// The words [w0, w1) of `in` (global) into `stage`, and zeros behind them up to PROBE_LDS_DW + WIDE_PAD_DW.  Whole workgroup.
__device__ void stage_words(const uint32_t *in, uint64_t nwords, uint64_t w0, uint64_t w1, uint32_t *stage) {
    for (uint32_t i = threadIdx.x; i < PROBE_LDS_DW + WIDE_PAD_DW; i += blockDim.x)
        stage[i] = (w0 + i < w1 && w0 + i < nwords) ? in[w0 + i] : 0u;
    __syncthreads();
}

// The workgroup's stream range: the lowest start word and the highest end word of its lanes (a wave of 64 lanes a workgroup)
__device__ void lane_range(uint64_t start, uint64_t end, bool act, uint64_t *w0, uint64_t *w1) {
    uint64_t lo = act ? start >> 5 : ~0ull, hi = act ? (end + 31) >> 5 : 0;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t l2 = (uint64_t)__shfl_xor((long long)lo, d, 64), h2 = (uint64_t)__shfl_xor((long long)hi, d, 64);
        lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
    }
    *w0 = lo; *w1 = hi;
}

// ------------------------------------------------------------------ probe_values
// lane i: nvals values at rung[i] from bit start[i] (stream end at end[i]); rung 0 reads the rung-0 form (a flag, sixteen bits
// when it is set) as one value.  out[i * (nvals + 1) + k]: value k (unswapped), then the bit behind the last one.
template <typename T, typename PTR>
__device__ void read_values(ReaderT<PTR> &rd, uint32_t r, uint32_t nvals, uint64_t *o) {
    for (uint32_t k = 0; k < nvals; k++) {
        uint64_t v;
        if (r == 0) v = rd.get(1) ? rd.get(16) : 0;
        else v = (uint64_t)unswap<T>(get_value<T, ReaderT<PTR>>(rd, r), r);
        o[k] = v;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void probe_values_kernel(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                         const uint32_t *rung, uint32_t nlanes, uint32_t nvals, uint32_t lds, uint64_t *out) {
    __shared__ uint32_t stage[PROBE_LDS_DW + WIDE_PAD_DW];
    const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
    const bool act = lane < nlanes;
    const uint64_t e = act ? (end[lane] < 32 * nwords ? end[lane] : 32 * nwords) : 0, s = act ? (start[lane] < e ? start[lane] : e) : 0;
    const uint32_t r = act ? rung[lane] % (8 * sizeof(T)) : 0;
    uint64_t *o = out + (uint64_t)lane * (nvals + 1);
    if (lds) {
        uint64_t w0, w1;
        lane_range(s, e, act, &w0, &w1);
        if (w1 > w0 && w1 - w0 > PROBE_LDS_DW) { if (act) o[nvals] = PROBE_TOO_BIG; return; }
        stage_words(in, nwords, w0, w1, stage);
        if (!act) return;
        ReaderT<LdsWords> rd;
        rd.init((LdsWords)stage, s - 32 * w0, e - 32 * w0);
        read_values<T, LdsWords>(rd, r, nvals, o);
        o[nvals] = rd.position() + 32 * w0;
    } else {
        if (!act) return;
        ReaderT<const uint32_t *> rd;
        rd.init(in, s, e);
        read_values<T, const uint32_t *>(rd, r, nvals, o);
        o[nvals] = rd.position();
    }
}

// ------------------------------------------------------------------ probe_groups
// lane i: one group of sixteen values at rung[i] from bit start[i] (stream end at end[i]) through
//   path 0: get_group<T, STEP> (ReaderT over global memory, or over the staged words when lds)
//   path 1: dec3_group<T, STEP, PTR, false>  (the sixteen values come out accumulated: run[k] = sum of smag of the first k + 1)
//   path 2: dec3_group<T, STEP, LdsWords, true>  (32/64-bit, staged words)
//   path 3: wide_values_lds<T, STEP>  (32/64-bit, staged words, rungs 8 and above)
// out[i * 17 + k]: value k, then the bit behind the group.
template <typename T, bool STEP, typename PTR>
__device__ void group_at(PTR src, uint64_t s, uint64_t e, uint32_t r, uint32_t path, const uint16_t *dtab, uint64_t *o) {
    T g[16];
    uint64_t endbit = 0;
    if (path == 0) {
        ReaderT<PTR> rd;
        rd.init(src, s, e);
        get_group<T, STEP, ReaderT<PTR>>(rd, r, g);
        endbit = rd.position();
    } else {
        uint32_t eb = 0;
        dec3_group<T, STEP, PTR, false>(src, (uint32_t)((e + 31) >> 5), (uint32_t)s, r, dtab, g, &eb);
        endbit = eb;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) o[k] = (uint64_t)g[k];
    o[16] = endbit;
}

template <typename T, bool STEP>
__device__ void group_window(LdsWords src, uint32_t s, uint32_t e, uint32_t r, uint32_t path, const uint16_t *dtab, uint64_t *o) {
    if constexpr (sizeof(T) >= 4) {
        T g[16];
        uint32_t eb = 0;
        if (path == 2) dec3_group<T, STEP, LdsWords, true>(src, (e + 31) >> 5, s, r, dtab, g, &eb);
        else if (r) wide_values_lds<T, STEP>(src, s, r, g, &eb);
        else {
#pragma unroll
            for (int k = 0; k < 16; k++) g[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < 16; k++) o[k] = (uint64_t)g[k];
        o[16] = eb;
    }
}

template <typename T, bool STEP>
__global__ __launch_bounds__(64) void probe_groups_kernel(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                         const uint32_t *rung, uint32_t nlanes, uint32_t path, uint32_t lds, uint64_t *out) {
    __shared__ uint32_t stage[PROBE_LDS_DW + WIDE_PAD_DW];
    __shared__ uint16_t dtab[DEC_TAB_SIZE];
    fill_dec_tab(dtab);
    __syncthreads();
    const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
    const bool act = lane < nlanes;
    const uint64_t e = act ? (end[lane] < 32 * nwords ? end[lane] : 32 * nwords) : 0, s = act ? (start[lane] < e ? start[lane] : e) : 0;
    const uint32_t r = act ? rung[lane] % (8 * sizeof(T)) : 0;
    uint64_t *o = out + (uint64_t)lane * 17;
    if (!lds && path < 2) {
        if (act) group_at<T, STEP, const uint32_t *>(in, s, e, r, path, dtab, o);
        return;
    }
    uint64_t w0, w1;
    lane_range(s, e, act, &w0, &w1);
    if (w1 > w0 && w1 - w0 > PROBE_LDS_DW) { if (act) o[16] = PROBE_TOO_BIG; return; }
    stage_words(in, nwords, w0, w1, stage);
    if (!act) return;
    const uint32_t rs = (uint32_t)(s - 32 * w0), re = (uint32_t)(e - 32 * w0);
    if (path < 2) group_at<T, STEP, LdsWords>((LdsWords)stage, rs, re, r, path, dtab, o);
    else group_window<T, STEP>((LdsWords)stage, rs, re, r, path, dtab, o);
    o[16] += 32 * w0;
}

// ------------------------------------------------------------------ probe_units
// Workgroup i: lane 0 decodes the unit stream of a one-band raster of w x 4 values at bits [start[i], end[i]) through parse_unit,
// keeping rung and factor as the kernels do (from rung 0, factor 0, entering value 0: the coder's state after a reset), and
// accumulates each unit along the curve into out + i * 4 * w (row-major w x 4).  ok[i]: 1 when every unit parsed and the last one
// ended at end[i], 0 if not, PROBE_TOO_BIG when the range did not fit the staging.
template <typename T, int MODE, typename PTR>
__device__ uint32_t decode_units(PTR src, uint64_t s, uint64_t e, uint32_t w, uint64_t order, T *img) {
    ReaderT<PTR> rd;
    rd.init(src, s, e);
    uint32_t rung = 0;
    T pcf = 0, prev = 0, g[16];
    bool ok = true;
    for (uint32_t bx = 0; bx < w / 4; bx++) {
        ok = parse_unit<T, MODE, ReaderT<PTR>>(rd, rung, pcf, g) && ok;
#pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            prev = (T)(prev + smag_t<T>(g[i]));
            const uint32_t nib = curve_nib(order, i);
            img[(nib >> 2) * w + 4 * bx + (nib & 3)] = prev;
        }
    }
    return ok && rd.position() == e ? 1u : 0u;
}

template <typename T, typename PTR>
__device__ uint32_t decode_units_mode(PTR src, uint64_t s, uint64_t e, uint32_t w, uint32_t mode, T *img) {
    if (mode == CM_FTL) return decode_units<T, CM_FTL, PTR>(src, s, e, w, HILBERT, img);
    if (mode == CM_BASE) return decode_units<T, CM_BASE, PTR>(src, s, e, w, HILBERT, img);
    return decode_units<T, CM_BEST, PTR>(src, s, e, w, HILBERT, img);
}

template <typename T>
__global__ __launch_bounds__(64) void probe_units_kernel(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                        uint32_t ncopies, uint32_t w, uint32_t mode, uint32_t lds, T *out, uint32_t *ok) {
    __shared__ uint32_t stage[PROBE_LDS_DW + WIDE_PAD_DW];
    const uint32_t c = blockIdx.x;
    if (c >= ncopies) return;
    const uint64_t e = end[c] < 32 * nwords ? end[c] : 32 * nwords, s = start[c] < e ? start[c] : e;
    T *img = out + (uint64_t)c * 4 * w;
    if (lds) {
        const uint64_t w0 = s >> 5, w1 = (e + 31) >> 5;
        if (w1 - w0 > PROBE_LDS_DW) { if (threadIdx.x == 0) ok[c] = PROBE_TOO_BIG; return; }
        stage_words(in, nwords, w0, w1, stage);
        if (threadIdx.x == 0) ok[c] = decode_units_mode<T, LdsWords>((LdsWords)stage, s - 32 * w0, e - 32 * w0, w, mode, img);
    } else if (threadIdx.x == 0) {
        ok[c] = decode_units_mode<T, const uint32_t *>(in, s, e, w, mode, img);
    }
}

// ------------------------------------------------------------------ probe_dirty
// Every workgroup takes all the dynamic LDS a workgroup may have and fills it with `pattern`, and every lane keeps DIRTY_REGS
// registers live holding it (each pinned by empty asm statements, in one order and back, so that each is a register of its own and all are
// live at once), then reads some of the
// LDS back.  The only global write: each wave's checksum, one vector store into out[(workgroup * 8 + wave) % nout].
__global__ __launch_bounds__(512) void probe_dirty_kernel(uint32_t pattern, uint32_t lds_words, uint32_t *out, uint32_t nout) {
    extern __shared__ uint32_t junk[];
    for (uint32_t i = threadIdx.x; i < lds_words; i += blockDim.x) junk[i] = pattern;
    uint32_t x[DIRTY_REGS];
#pragma unroll
    for (int i = 0; i < DIRTY_REGS; i++) {
        x[i] = pattern;
        asm volatile("" : "+v"(x[i]));
    }
#pragma unroll
    for (int i = DIRTY_REGS - 1; i >= 0; i--) asm volatile("" : "+v"(x[i]));     // (the first one defined is the last one touched: all live at once)
    __syncthreads();
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < DIRTY_REGS; i++) acc += x[i] ^ (uint32_t)i;
    for (uint32_t i = (threadIdx.x * 97u) % lds_words, k = 0; k < 4; k++, i = (i + 4099u) % lds_words) acc += junk[i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += (uint32_t)__shfl_xor((int)acc, d, 64);
    if ((threadIdx.x & 63) == 0) out[(blockIdx.x * 8 + (threadIdx.x >> 6)) % nout] = acc;
}

template <typename T>
int launch_values(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end, const uint32_t *rung, uint32_t nlanes,
                  uint32_t nvals, uint32_t lds, uint64_t *out, hipStream_t st) {
    hipLaunchKernelGGL(probe_values_kernel<T>, dim3((nlanes + 63) / 64), dim3(64), 0, st, in, nwords, start, end, rung, nlanes, nvals, lds, out);
    return (int)hipGetLastError();
}

template <typename T>
int launch_groups(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end, const uint32_t *rung, uint32_t nlanes,
                  uint32_t step, uint32_t path, uint32_t lds, uint64_t *out, hipStream_t st) {
    const dim3 grid((nlanes + 63) / 64), blk(64);
    if (step) hipLaunchKernelGGL((probe_groups_kernel<T, true>), grid, blk, 0, st, in, nwords, start, end, rung, nlanes, path, lds, out);
    else hipLaunchKernelGGL((probe_groups_kernel<T, false>), grid, blk, 0, st, in, nwords, start, end, rung, nlanes, path, lds, out);
    return (int)hipGetLastError();
}

template <typename T>
int launch_units(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end, uint32_t ncopies, uint32_t w,
                 uint32_t mode, uint32_t lds, void *out, uint32_t *ok, hipStream_t st) {
    hipLaunchKernelGGL(probe_units_kernel<T>, dim3(ncopies), dim3(64), 0, st, in, nwords, start, end, ncopies, w, mode, lds, (T *)out, ok);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// width: bytes per value (1, 2, 4, 8).  Returns 0, or a HIP error code, or -1 for arguments the probe does not take.
__attribute__((visibility("default"))) int probe_values(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                        const uint32_t *rung, uint32_t nlanes, uint32_t nvals, uint32_t width, uint32_t lds,
                                                        uint64_t *out, hipStream_t st) {
    if (!nlanes || !nvals) return -1;
    switch (width) {
    case 1: return launch_values<uint8_t>(in, nwords, start, end, rung, nlanes, nvals, lds, out, st);
    case 2: return launch_values<uint16_t>(in, nwords, start, end, rung, nlanes, nvals, lds, out, st);
    case 4: return launch_values<uint32_t>(in, nwords, start, end, rung, nlanes, nvals, lds, out, st);
    case 8: return launch_values<uint64_t>(in, nwords, start, end, rung, nlanes, nvals, lds, out, st);
    }
    return -1;
}

// path 0 get_group, 1 dec3_group (no window), 2 dec3_group with the window (lds, width 4 / 8), 3 wide_values_lds (lds, width 4 / 8)
__attribute__((visibility("default"))) int probe_groups(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                        const uint32_t *rung, uint32_t nlanes, uint32_t width, uint32_t step, uint32_t path,
                                                        uint32_t lds, uint64_t *out, hipStream_t st) {
    if (!nlanes || path > 3 || (path >= 2 && (!lds || width < 4))) return -1;
    switch (width) {
    case 1: return launch_groups<uint8_t>(in, nwords, start, end, rung, nlanes, step, path, lds, out, st);
    case 2: return launch_groups<uint16_t>(in, nwords, start, end, rung, nlanes, step, path, lds, out, st);
    case 4: return launch_groups<uint32_t>(in, nwords, start, end, rung, nlanes, step, path, lds, out, st);
    case 8: return launch_groups<uint64_t>(in, nwords, start, end, rung, nlanes, step, path, lds, out, st);
    }
    return -1;
}

// mode: 0 FTL, 1 BASE, 2 BEST (qb3_dev.h CodecMode); w a multiple of 4; out: ncopies rasters of w x 4 values of `width` bytes
__attribute__((visibility("default"))) int probe_units(const uint32_t *in, uint64_t nwords, const uint64_t *start, const uint64_t *end,
                                                       uint32_t ncopies, uint32_t w, uint32_t width, uint32_t mode, uint32_t lds,
                                                       void *out, uint32_t *ok, hipStream_t st) {
    if (!ncopies || !w || (w & 3) || mode > 2) return -1;
    switch (width) {
    case 1: return launch_units<uint8_t>(in, nwords, start, end, ncopies, w, mode, lds, out, ok, st);
    case 2: return launch_units<uint16_t>(in, nwords, start, end, ncopies, w, mode, lds, out, ok, st);
    case 4: return launch_units<uint32_t>(in, nwords, start, end, ncopies, w, mode, lds, out, ok, st);
    case 8: return launch_units<uint64_t>(in, nwords, start, end, ncopies, w, mode, lds, out, ok, st);
    }
    return -1;
}

// out: nout words the checksums land in (nout >= 1)
__attribute__((visibility("default"))) int probe_dirty(uint32_t pattern, uint32_t *out, uint32_t nout, hipStream_t st) {
    if (!nout) return -1;
    int dev = 0, cus = 0, lds = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e != hipSuccess) return (int)e;
    if (cus <= 0 || lds < 4) return -1;
    e = hipFuncSetAttribute((const void *)probe_dirty_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (e != hipSuccess) return (int)e;
    // the LDS of a workgroup fills a CU: one workgroup a CU at a time, twice as many as there are CUs
    hipLaunchKernelGGL(probe_dirty_kernel, dim3(2 * cus), dim3(512), (size_t)lds, st, pattern, (uint32_t)(lds / 4), out, nout);
    return (int)hipGetLastError();
}

}  // extern "C"
