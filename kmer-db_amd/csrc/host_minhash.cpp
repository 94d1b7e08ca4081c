// host_minhash.cpp — <sample>.minhash files (front-end, CPU): the reader and the writer of the reference's MihashedInputFile
// (src/minhashed_input_file.h:58-118).
//
// The format is 24 bytes of framing around a sorted list, every field little-endian and unpadded as the reference's x86-64 build writes it:
//   u32 signature 0xfedcba98 | u64 count | count x u64 k-mer words | u32 k-mer length | f64 fraction
#include "kmdb_amd.h"
#include "kmdb_internal.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <sys/stat.h>

namespace {
constexpr uint32_t MINHASH_FORMAT_SIGNATURE = 0xfedcba98u;
static_assert(sizeof(size_t) == 8 && sizeof(double) == 8, "the file holds the reference's size_t and double");
struct File {
    FILE* f = nullptr;
    ~File() { if (f) std::fclose(f); }
};
}  // namespace

// MihashedInputFile::store (minhashed_input_file.h:109-118; console_minhash.cpp:47)
extern "C" int kmdbh_minhash_store(const char* path, const uint64_t* kmers, size_t count, uint32_t kmer_length, double fraction) {
    if (!path || (count && !kmers)) return kmdb_set_error("kmdbh_minhash_store: null argument");
    File o;
    o.f = std::fopen(path, "wb");
    if (!o.f) return kmdb_set_error(std::string("kmdbh_minhash_store: cannot write ") + path);
    const uint64_t n = count;
    bool ok = std::fwrite(&MINHASH_FORMAT_SIGNATURE, 4, 1, o.f) == 1 && std::fwrite(&n, 8, 1, o.f) == 1;
    ok = ok && (count == 0 || std::fwrite(kmers, 8, count, o.f) == count);
    ok = ok && std::fwrite(&kmer_length, 4, 1, o.f) == 1 && std::fwrite(&fraction, 8, 1, o.f) == 1;
    const int rc = std::fclose(o.f);
    o.f = nullptr;
    if (!ok || rc) return kmdb_set_error(std::string("kmdbh_minhash_store: cannot write ") + path);
    return 0;
}

// MihashedInputFile::open + load (minhashed_input_file.h:58-105; console_one2all.cpp:57)
extern "C" int kmdbh_minhash_load(const char* path, uint64_t** kmers, size_t* count, uint32_t* kmer_length, double* fraction) {
    if (!path || !kmers || !count) return kmdb_set_error("kmdbh_minhash_load: null argument");
    *kmers = nullptr; *count = 0;
    File in;
    in.f = std::fopen(path, "rb");
    if (!in.f) return kmdb_set_error(std::string("kmdbh_minhash_load: cannot open ") + path);
    struct stat sb{};
    if (fstat(fileno(in.f), &sb) || !S_ISREG(sb.st_mode)) return kmdb_set_error(std::string("kmdbh_minhash_load: not a regular file: ") + path);
    const uint64_t size = (uint64_t)sb.st_size;
    uint32_t signature = 0;
    uint64_t n = 0;
    if (size < 24 || std::fread(&signature, 4, 1, in.f) != 1 || std::fread(&n, 8, 1, in.f) != 1)
        return kmdb_set_error(std::string("kmdbh_minhash_load: truncated file ") + path);
    if (signature != MINHASH_FORMAT_SIGNATURE) return kmdb_set_error(std::string("kmdbh_minhash_load: not a minhash file (wrong signature): ") + path);
    // the count against the file's size, before anything is allocated
    if (n > (size - 24) / 8 || 24 + 8 * n != size)
        return kmdb_set_error(std::string("kmdbh_minhash_load: the k-mer count does not agree with the size of ") + path);
    uint64_t* buf = (uint64_t*)std::malloc(n ? n * 8 : 8);
    if (!buf) return kmdb_set_error("kmdbh_minhash_load: out of host memory");
    uint32_t k = 0;
    double f = 0;
    if ((n && std::fread(buf, 8, n, in.f) != n) || std::fread(&k, 4, 1, in.f) != 1 || std::fread(&f, 8, 1, in.f) != 1) {
        std::free(buf);
        return kmdb_set_error(std::string("kmdbh_minhash_load: truncated file ") + path);
    }
    *kmers = buf; *count = (size_t)n;
    if (kmer_length) *kmer_length = k;
    if (fraction) *fraction = f;
    return 0;
}

extern "C" void kmdbh_minhash_free(uint64_t* kmers) { std::free(kmers); }
