// tools/qb3index.cpp -- gives a QB3 container that exists a restart table (or takes it away) without coding its stream again:
// the command line caller of qb3x_reindex (include/qb3x.h).  Every byte behind "DT" stays as it is; the reference's decoder steps
// over the table's chunks (QB3decode.cpp:251-255), this library's decodes from them in parallel and reads windows.
//
//   qb3index [-0|-1|-2] [-v] in.qb3 out.qb3
//
//   -0 no table (the reference's bytes)   -1 positions and states   -2 with block / unit lengths (the default)
//   -v prints sizes, table entries and milliseconds
#include "qb3x.h"
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {

int fail(const std::string &msg) {
    fprintf(stderr, "qb3index: %s\n", msg.c_str());
    return 1;
}

bool read_file(const std::string &name, std::vector<uint8_t> &v) {
    FILE *f = fopen(name.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    bool ok = n >= 0;
    if (ok) { v.resize((size_t)n); ok = n == 0 || fread(v.data(), 1, (size_t)n, f) == (size_t)n; }
    fclose(f);
    return ok;
}

bool write_file(const std::string &name, const uint8_t *p, size_t n) {
    FILE *f = fopen(name.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, n, f) == n;
    return fclose(f) == 0 && ok;
}

// table entries the decoder finds in a container (0: none)
size_t table_entries(std::vector<uint8_t> &c, size_t n) {
    size_t dims[3];
    decsp d = qb3_read_start(c.data(), n, dims);
    size_t k = 0;
    if (d) { if (qb3_read_info(d)) k = qb3x_decoder_table_entries(d); qb3_destroy_decoder(d); }
    return k;
}

}  // namespace

int main(int argc, char **argv) {
    int level = 2;
    bool verbose = false;
    std::vector<std::string> names;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-0" || a == "-1" || a == "-2") level = a[1] - '0';
        else if (a == "-v") verbose = true;
        else if (!a.empty() && a[0] == '-') { fprintf(stderr, "qb3index [-0|-1|-2] [-v] in.qb3 out.qb3\n"); return 2; }
        else names.push_back(a);
    }
    if (names.size() != 2) { fprintf(stderr, "qb3index [-0|-1|-2] [-v] in.qb3 out.qb3\n"); return 2; }
    std::vector<uint8_t> src;
    if (!read_file(names[0], src)) return fail("cannot read " + names[0]);
    size_t dims[3];
    decsp d = qb3_read_start(src.data(), src.size(), dims);
    if (!d || !qb3_read_info(d)) { if (d) qb3_destroy_decoder(d); return fail(names[0] + " is not a QB3 container"); }
    const size_t bound = qb3x_reindex_size(d, level), had = qb3x_decoder_table_entries(d);
    qb3_destroy_decoder(d);
    if (!bound) return fail("cannot size the output");
    std::vector<uint8_t> dst(bound);
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = qb3x_reindex(src.data(), src.size(), dst.data(), dst.size(), level);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (!n) return fail(std::string("reindex failed: ") + qb3x_last_error());
    if (!write_file(names[1], dst.data(), n)) return fail("cannot write " + names[1]);
    if (verbose)
        printf("%zu x %zu x %zu: %zu bytes, %zu table entries -> level %d: %zu bytes, %zu table entries, %.2f ms\n", dims[0], dims[1], dims[2],
               src.size(), had, level, n, table_entries(dst, n), ms);
    return 0;
}
