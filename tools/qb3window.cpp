// tools/qb3window.cpp -- a rectangle of a QB3 file as a PNM image, reading only the bytes of the file that hold it: the command line
// caller of qb3x_open_ranged / qb3x_read_windows_ranged (include/qb3x.h), with pread as the reader.  A file with a level-2 restart
// table (cqb3x with QB3X_INDEX_CHUNK=2, qb3index -2) is read in pieces -- an 8-bit FTL / BASE one always, a 16-bit one with -k, an
// 8-bit common-factor one with -K; any other file is read whole and gives the same pixels.
//
//   qb3window [-v] [-k] [-K] [-u] [-U] [-g gap] [-b bands] in.qb3 x0,y0,w,h out.pnm
//
//   -b list chosen bands of the window, comma separated (one or three of them: 3,2,1 of an eight-band file as a false-colour image):
//           qb3x_read_windows_bands.  Band selection is not built for the ranged calls, so the file is then read whole into memory;
//           with -u / -U the lane-per-unit window kernels write the chosen bands themselves
//   -g gap  merge two byte ranges that lie at most `gap` bytes apart (fewer reads, more bytes; default 0)
//   -k      16-bit files too are read in pieces (qb3x_set_decoder_window_kernels, QB3X_WINK_U16)
//   -K      8-bit files of 1, 3, 4 bands in the common-factor modes (cqb3x -b, qb3tiles -b) too are read in pieces (QB3X_WINK_CF8);
//           without it such a file is read whole
//   -u      sets QB3X_WINK_UNIT: no file is read in pieces for it, but the window of a file the lane-per-unit window kernels take (a
//           32-bit one-band file, say) is then decoded by them from the file read whole, not through a raster-sized scratch buffer
//   -U      sets QB3X_WINK_CFU: the same for the common-factor modes of such files (a 16-bit grey or RGB file written with cqb3x -b, say)
//   -v      prints bytes read and calls of the reader against the file's size
#include "qb3x.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

namespace {

const char *USAGE = "qb3window [-v] [-k] [-K] [-u] [-U] [-g gap] [-b bands] in.qb3 x0,y0,w,h out.pnm\n"
                    "  -b  comma separated band numbers: write these bands of the window (the file is read whole)\n"
                    "  -k  read 16-bit files in pieces too    -K  read 8-bit common-factor files (cqb3x -b) in pieces too\n"
                    "  -u  window kernels for files read whole (QB3X_WINK_UNIT)\n"
                    "  -U  ... and for their common-factor modes (QB3X_WINK_CFU)\n";

int fail(const std::string &msg) {
    fprintf(stderr, "qb3window: %s\n", msg.c_str());
    return 1;
}

// qb3x_read_fn over a file descriptor
int read_at(void *ctx, uint64_t offset, void *dst, size_t size) {
    const int fd = *(const int *)ctx;
    uint8_t *to = (uint8_t *)dst;
    while (size) {
        const ssize_t got = pread(fd, to, size, (off_t)offset);
        if (got <= 0) return 1;
        to += got; offset += (uint64_t)got; size -= (size_t)got;
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    bool verbose = false, kernels16 = false, kernels_cf = false, kernels_unit = false, kernels_cfu = false;
    size_t gap = 0;
    std::vector<uint8_t> sel;
    bool bands_given = false;
    std::vector<std::string> names;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-v") verbose = true;
        else if (a == "-k") kernels16 = true;
        else if (a == "-K") kernels_cf = true;
        else if (a == "-u") kernels_unit = true;
        else if (a == "-U") kernels_cfu = true;
        else if (a == "-g" && i + 1 < argc) gap = (size_t)strtoull(argv[++i], nullptr, 10);
        else if (a == "-b" && i + 1 < argc) {
            bands_given = true;
            for (const char *q = argv[++i]; *q;) {
                char *end = nullptr;
                const unsigned long v = strtoul(q, &end, 10);
                if (end == q || v > 255 || (*end && *end != ',')) { fputs(USAGE, stderr); return 2; }
                sel.push_back((uint8_t)v);
                q = *end ? end + 1 : end;
            }
        }
        else if (!a.empty() && a[0] == '-') { fputs(USAGE, stderr); return 2; }
        else names.push_back(a);
    }
    unsigned long long x0, y0, w, h;
    if (names.size() != 3 || sscanf(names[1].c_str(), "%llu,%llu,%llu,%llu", &x0, &y0, &w, &h) != 4) { fputs(USAGE, stderr); return 2; }
    int fd = open(names[0].c_str(), O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0) return fail("cannot read " + names[0]);
    size_t dims[3];
    std::vector<uint8_t> whole;                         // -b: the file, read whole (the handle points into it)
    if (bands_given) {
        whole.resize((size_t)sb.st_size);
        if (whole.empty() || read_at(&fd, 0, whole.data(), whole.size())) { close(fd); return fail("cannot read " + names[0]); }
    }
    decsp d = bands_given ? qb3_read_start(whole.data(), whole.size(), dims) : qb3x_open_ranged(read_at, &fd, (uint64_t)sb.st_size, dims);
    if (d && bands_given && !qb3_read_info(d)) { qb3_destroy_decoder(d); d = nullptr; }
    if (!d) { close(fd); return fail(names[0] + " is not a QB3 container"); }
    const size_t nout = bands_given ? sel.size() : dims[2];      // bands of the image
    const qb3_dtype type = qb3_get_type(d);
    const size_t tsz = type <= QB3_I8 ? 1 : type <= QB3_I16 ? 2 : type <= QB3_I32 ? 4 : 8;
    int ret = 0;
    if ((nout != 1 && nout != 3) || tsz > 2) ret = fail("a PNM image holds one or three bands of 8 or 16 bits");
    else if (!w || !h || x0 >= dims[0] || w > dims[0] - x0 || y0 >= dims[1] || h > dims[1] - y0) ret = fail("the window is not inside the raster");
    else {
        std::vector<uint8_t> pix(w * h * nout * tsz);
        const qb3x_window win = { (size_t)x0, (size_t)y0, (size_t)w, (size_t)h, pix.data(), 0 };
        if (!bands_given) qb3x_set_ranged_gap(d, gap);
        qb3x_set_decoder_window_kernels(d, (kernels16 ? QB3X_WINK_U16 : 0u) | (kernels_cf ? QB3X_WINK_CF8 : 0u) | (kernels_unit ? QB3X_WINK_UNIT : 0u) | (kernels_cfu ? QB3X_WINK_CFU : 0u));
        if ((bands_given ? qb3x_read_windows_bands(d, &win, 1, sel.data(), sel.size()) : qb3x_read_windows_ranged(d, &win, 1)) != 1) ret = fail(std::string("the window was not read: ") + qb3x_last_error());
        else {
            if (tsz == 2) for (size_t i = 0; i + 1 < pix.size(); i += 2) std::swap(pix[i], pix[i + 1]);     // PNM samples are big endian
            FILE *f = fopen(names[2].c_str(), "wb");
            bool ok = f != nullptr;
            if (ok) {
                fprintf(f, "P%d\n%llu %llu\n%d\n", nout == 1 ? 5 : 6, w, h, tsz == 1 ? 255 : 65535);
                ok = fwrite(pix.data(), 1, pix.size(), f) == pix.size();
                ok = fclose(f) == 0 && ok;
            }
            if (!ok) ret = fail("cannot write " + names[2]);
            else if (verbose && bands_given)
                printf("%zu x %zu x %zu: %zu band(s) of window %llu,%llu,%llu,%llu on path %d, %zu gather launch(es); the file was read whole\n", dims[0], dims[1], dims[2],
                       nout, x0, y0, w, h, qb3x_last_window_path(d), qb3x_last_window_gathers(d));
            else if (verbose)
                printf("%zu x %zu x %zu: window %llu,%llu,%llu,%llu on path %d: %llu bytes in %llu reads of %lld (%.2f %%)\n", dims[0], dims[1], dims[2], x0, y0, w, h,
                       qb3x_last_window_path(d), (unsigned long long)qb3x_ranged_bytes(d), (unsigned long long)qb3x_ranged_reads(d), (long long)sb.st_size,
                       100.0 * (double)qb3x_ranged_bytes(d) / (double)sb.st_size);
        }
    }
    qb3_destroy_decoder(d);
    close(fd);
    return ret;
}
