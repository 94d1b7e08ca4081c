// ref_extract.cpp — ORACLE INFRASTRUCTURE (not product code).
//
// The reference's OWN k-mer extractor as a witness for the three restatements of this project (kmdb_oracle.c,
// csrc/host_kmers.cpp, csrc/new2all.hip).  This file is our driver code and only CALLS the reference's public headers, compiled
// from where they lie under $(REF)/src with the reference's build flags (oracle/Makefile: REF_CXXFLAGS):
//   KmerHelper::extract<MinHashFilter>            (kmer_extract.h:12-97)
//   AlphabetFactory::instance().create(name)      (alphabet.h:76-127)
//   FilterFactory::create(fraction, start, k)     (filter.h:136-146; a NullFilter is a MinHashFilter whose non-virtual operator() the
//                                                  call below does not reach, so fraction >= 1 keeps every k-mer here as the loader's
//                                                  NullFilter instantiation does)
// No reference file is copied or edited.  What the headers expect to be in scope before them (the reference's loader translation
// units provide it) is provided here: types.h before kmer_extract.h, <memory> / <string> / using namespace std, a FORCE_INLINE
// definition (elias_gamma.h:15) and the header-only sort of $(REF)/libs/refresh that KmerHelper::sort names.
//
// Usage:  ref_extract <alphabet name> <k> <fraction> <start fraction> <records.bin> <out.bin>
//   records.bin: per record u64 length, then the bytes          out.bin: per record u64 count, then count x u64 k-mer words
// One JSON line on stdout: the records and k-mers written and "lo" / "hi", the thresholds of the reference's filter object (as strings).
// The words are written IN EXTRACTION ORDER (no sort, no unique: the caller does both).  fraction and start are parsed with strtod, so
// the caller passes them with 17 significant digits or as C99 hex floats and the doubles arrive bit for bit.
//
// Inputs must be 7-bit ASCII: Alphabet::map(char) (alphabet.h:68) indexes its 256-entry table with a plain (signed) char, so a byte
// >= 0x80 reads in front of the table.  The driver refuses such a record instead of letting the reference read outside it.
// KmerHelper::extract reads the first k-1 symbols before it looks at the length (kmer_extract.h:48-58): every record is copied into a
// buffer padded with k zero bytes, so a record shorter than k-1 is safe to pass on (it yields no k-mer).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>
using namespace std;

#ifndef FORCE_INLINE
#define FORCE_INLINE inline __attribute__((always_inline))
#endif
#include "types.h"
#include "../libs/refresh/sort/lib/pdqsort_par.h"
#include "filter.h"
#include "kmer_extract.h"

// the thresholds the reference's filter object holds (protected members, read through a copy of the object FilterFactory made)
struct WindowPeek : MinHashFilter {
    explicit WindowPeek(const MinHashFilter& f) : MinHashFilter(f) {}
    uint64_t lo() const { return minThreshold; }
    uint64_t hi() const { return maxThreshold; }
};

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: ref_extract <alphabet> <k> <fraction> <start> <records.bin> <out.bin>\n"); return 2; }
    try {
        std::unique_ptr<Alphabet> alphabet(AlphabetFactory::instance().create(std::string(argv[1])));
        const uint32_t k = (uint32_t)strtoul(argv[2], nullptr, 10);
        const double fraction = strtod(argv[3], nullptr), start = strtod(argv[4], nullptr);
        if (k == 0 || (int)k > alphabet->maxKmerLen) { fprintf(stderr, "k must be 1..%d for %s\n", alphabet->maxKmerLen, argv[1]); return 1; }
        std::unique_ptr<MinHashFilter> filter(FilterFactory::create(fraction, start, (int)k));
        const bool all = !(fraction < 1.0);                    // FilterFactory made a NullFilter: the loader instantiates extract<NullFilter>
        FILE* in = fopen(argv[5], "rb");
        FILE* out = fopen(argv[6], "wb");
        if (!in || !out) { fprintf(stderr, "cannot open %s / %s\n", argv[5], argv[6]); return 1; }
        std::vector<char> seq;
        std::vector<kmer_t> kmers;
        uint64_t len = 0, records = 0, total = 0;
        while (fread(&len, 8, 1, in) == 1) {
            seq.assign(len + k + 1, 0);
            if (len && fread(seq.data(), 1, len, in) != len) { fprintf(stderr, "short record in %s\n", argv[5]); return 1; }
            for (uint64_t i = 0; i < len; ++i)
                if ((unsigned char)seq[i] >= 0x80) { fprintf(stderr, "record %llu: byte >= 0x80 (7-bit ASCII only)\n", (unsigned long long)records); return 1; }
            kmers.assign(len + 1, 0);
            const uint64_t n = all ? KmerHelper::extract(seq.data(), (size_t)len, k, *alphabet, static_cast<const NullFilter&>(*filter), kmers.data())
                                   : KmerHelper::extract(seq.data(), (size_t)len, k, *alphabet, *filter, kmers.data());
            fwrite(&n, 8, 1, out);
            if (n) fwrite(kmers.data(), 8, n, out);
            ++records; total += n;
        }
        fclose(in);
        if (fclose(out)) { fprintf(stderr, "cannot write %s\n", argv[6]); return 1; }
        const WindowPeek peek(*filter);
        printf("{\"cmd\":\"extract\",\"records\":%llu,\"kmers\":%llu,\"lo\":\"%llu\",\"hi\":\"%llu\"}\n", (unsigned long long)records, (unsigned long long)total,
               (unsigned long long)peek.lo(), (unsigned long long)peek.hi());
        return 0;
    } catch (const std::exception& e) {
        fprintf(stderr, "ref_extract: %s\n", e.what());
        return 1;
    }
}
