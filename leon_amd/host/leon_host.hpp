// leon_host.hpp -- host-side mirror (C++) of the reference interface AROUND the DNA encode path, above the C-ABI:
//   Leon      : the Tool-shaped class main() drives with `Leon().run(argc, argv)` (/root/reference/src/main.cpp:44);
//               run() parses the documented flags (/root/reference/README.md:38-58, -test-file: /root/reference/INSTALL:22)
//               and calls execute() -> executeCompression() / executeDecompression() [RECALLED names];
//   Exception : gatb::core::system::Exception's getMessage() contract (/root/reference/src/main.cpp:46-49).
// `-c` writes the `.leon` HDF5 container (leon_container.hpp) with the three streams Leon has -- headers, DNA,
// qualities -- and `-d` restores the FASTA / FASTQ file from it (the reference's acceptance test,
// /root/reference/scripts/simple_test.sh:51-62).  Every byte of the DNA and header streams comes from libleon_dna.so
// (HIP kernels); the quality stream is zlib on host threads (lossless) after a device smoothing pass (lossy, the default).
#pragma once
#include <stdint.h>
#include <exception>
#include <string>
#include <vector>

#include "../../include/leon_dna.h"

namespace leon_host {

class Exception : public std::exception {
public:
    explicit Exception(const std::string& m) : msg_(m) {}
    const char* getMessage() const { return msg_.c_str(); }
    const char* what() const noexcept override { return msg_.c_str(); }
private:
    std::string msg_;
};

class Container;

class Leon {
public:
    static const int READ_PER_BLOCK = 50000;
    static const char* STR_COMPRESS;      // "-c"
    static const char* STR_DECOMPRESS;    // "-d"
    Leon();
    ~Leon();
    void run(int argc, char* argv[]);     // Tool::run: parse, then execute()
    void execute();

    // options (upstream: members of Leon filled from the Tool's properties)
    std::string _inputFilename, _outputFilename;
    bool _compress = false, _decompress = false;
    size_t _kmerSize = 31;
    int _abundance = 0;                   // 0 = automatic (/root/reference/README.md:54)
    int _nbCores = 0;                     // 0 = all
    int _gpus = 1;
    bool _lossless = false, _seqOnly = false, _noHeader = false, _noQual = false, _testFile = false, _verbose = false;
    bool _checksum = false;               // -c: -checksum: a CRC-32 per read block and stream in leon/metadata/checksums; -d verifies it whenever it is there
    bool _ignoreChecksum = false;         // -d: -ignore-checksum: a mismatch is a WARNING on stderr, the file is kept
    bool _letters = false;                // -c: -letters: lower-case runs and bytes outside ACGTN kept in leon/metadata/letter_*; -d puts them back whenever they are there
    bool _gz = false;                     // -d: -gz: the restored file written as BGZF (X.d.gz), compressed on the device
    bool _gzRecords = false;              // -d -gz: -gz-records: the members cut at record starts
    bool _dictPieces = false;             // -c -dict-pieces: the anchor dictionary written as independently coded pieces, coded on the device
    uint32_t _dictPieceAnchors = 0;       // -c -dict-pieces -dict-piece-anchors N: anchors per piece (0: the library's default, 1024)
    bool _gzMatches = false;              // -d -gz: -gz-matches: LZ77 matches in the members, k_deflate_lz_chunks
    bool _gzIndex = false;                // -d -gz: -gz-index: X.d.gz.gzi beside the file, every member's offset in the file and in the text
    bool _bam = false;                    // -d: -bam: the restored reads as unaligned BAM (X.d.bam), records and BGZF written on the device
    std::string _qualDeflate;             // -qual-deflate host|device|auto; empty = not given: zlib on the host threads (the reference's bytes)
    std::string _inputInflate;            // -c: -input-inflate host|device|auto; empty = not given: a gzip input inflated by zlib on the reader's thread
    std::string _recordParse;             // -c: -record-parse host|device; empty = not given: the FASTQ records cut by the reader's thread on the host
    bool _recordParseFasta = false;       // -c -record-parse device: -record-parse-fasta, a FASTA input is split on the device too
    std::string _headerText;              // -d: -header-text host|device|auto; empty = not given: the header text on the host threads
    std::string _recordText;              // -d: -record-text host|device|auto; empty = not given: the records formatted on the host threads
    std::string _qualInflate;             // -d: -qual-inflate host|device|auto; empty = not given: the quality blocks inflated by zlib on the host threads

private:
    void executeCompression();
    void executeDecompression();
    void testDecompressedFile();
};

// `leon -selftest-container <path>` / `leon -selftest-bank <file>`: host logic that runs without a GPU (used by the CPU tests)
int selftest_container(const std::string& path);
int selftest_bank(const std::string& path);

}  // namespace leon_host
