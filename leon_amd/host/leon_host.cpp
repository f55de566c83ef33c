// leon_host.cpp -- see leon_host.hpp.  Host glue only: the DNA and header streams come from libleon_dna.so's HIP path.
// Here: the options, `-test-file` and the two self-tests; `-c` is leon_compress.cpp, `-d` is leon_decompress.cpp, what they share
// leon_internal.hpp.
#include "leon_internal.hpp"

#include "bank.hpp"

#include <fcntl.h>
#include <sys/stat.h>
#include <zlib.h>

#include <iostream>

namespace leon_host {

using namespace layout;

const char* Leon::STR_COMPRESS = "-c";
const char* Leon::STR_DECOMPRESS = "-d";

// ------------------------------------------------------------------------------------------------ Leon
Leon::Leon() {}
Leon::~Leon() {}

void Leon::run(int argc, char* argv[]) {
    try {
        for (int i = 1; i < argc; i++) {
            std::string a = argv[i];
            auto need = [&](const char* flag) -> std::string {
                if (i + 1 >= argc) throw Exception(std::string("option ") + flag + " needs a value");
                return argv[++i];
            };
            auto number = [&](const char* flag) -> long {
                const std::string v = need(flag);
                size_t used = 0;
                long x = 0;
                try { x = std::stol(v, &used); } catch (const std::exception&) { used = 0; }
                if (used != v.size() || v.empty()) throw Exception(std::string("option ") + flag + ": '" + v + "' is not a number");
                return x;
            };
            if (a == "-file") _inputFilename = need("-file");
            else if (a == STR_COMPRESS) _compress = true;
            else if (a == STR_DECOMPRESS) _decompress = true;
            else if (a == "-kmer-size") _kmerSize = (size_t)number("-kmer-size");
            else if (a == "-abundance") { _abundance = (int)number("-abundance"); if (_abundance < 1) throw Exception("-abundance must be at least 1"); }
            else if (a == "-nb-cores") _nbCores = (int)std::max<long>(0, number("-nb-cores"));
            else if (a == "-gpus") { _gpus = (int)number("-gpus"); if (_gpus < 1 || _gpus > 64) throw Exception("-gpus must be in 1..64"); }
            else if (a == "-verbose") _verbose = number("-verbose") != 0;
            else if (a == "-lossless") _lossless = true;
            else if (a == "-seq-only") _seqOnly = true;
            else if (a == "-noheader") _noHeader = true;
            else if (a == "-noqual") _noQual = true;
            else if (a == "-test-file") _testFile = true;
            else if (a == "-checksum") _checksum = true;
            else if (a == "-ignore-checksum") _ignoreChecksum = true;
            else if (a == "-letters") _letters = true;
            else if (a == "-gz") _gz = true;
            else if (a == "-gz-records") _gzRecords = true;
            else if (a == "-gz-index") _gzIndex = true;
            else if (a == "-gz-matches") _gzMatches = true;
            else if (a == "-bam") _bam = true;
            else if (a == "-dict-pieces") _dictPieces = true;
            else if (a == "-dict-piece-anchors") {
                const long v = number("-dict-piece-anchors");
                if (v < 1 || v > (1l << 20)) throw Exception("-dict-piece-anchors must be in 1..1048576");
                _dictPieceAnchors = (uint32_t)v;
            }
            else if (a == "-qual-deflate") { _qualDeflate = need("-qual-deflate"); (void)qual_encoder_choice(_qualDeflate); }
            else if (a == "-input-inflate") { _inputInflate = need("-input-inflate"); (void)parse_choice("-input-inflate", _inputInflate); }
            else if (a == "-record-parse") { _recordParse = need("-record-parse"); (void)record_parse_on_device(_recordParse); }
            else if (a == "-record-parse-fasta") _recordParseFasta = true;
            else if (a == "-header-text") { _headerText = need("-header-text"); (void)parse_choice("-header-text", _headerText); }
            else if (a == "-record-text") { _recordText = need("-record-text"); (void)parse_choice("-record-text", _recordText); }
            else if (a == "-qual-inflate") { _qualInflate = need("-qual-inflate"); (void)parse_choice("-qual-inflate", _qualInflate); }
            else throw Exception("unknown option " + a);
        }
        if (_inputFilename.empty()) throw Exception("option -file is mandatory");
        if (_compress == _decompress) throw Exception("choose one of -c (compress) or -d (decompress)");
        if (_checksum && _decompress) throw Exception("option -checksum belongs to -c: -d verifies whenever the container holds checksums (-ignore-checksum to go on past a mismatch)");
        if (_ignoreChecksum && _compress) throw Exception("option -ignore-checksum belongs to -d");
        if (_letters && _decompress) throw Exception("option -letters belongs to -c: -d restores the letters whenever the container holds them");
        if (_gz && _compress) throw Exception("option -gz belongs to -d");
        if (_bam && _compress) throw Exception("option -bam belongs to -d");
        if (_gz && _bam) throw Exception("options -gz and -bam name two output formats");
        // (-bam takes the three -gz-* options as -gz does; the words of their refusal are as they were)
        if (_gzRecords && !_gz && !_bam) throw Exception("option -gz-records belongs to -gz");
        if (_gzIndex && !_gz && !_bam) throw Exception("option -gz-index belongs to -gz");
        if (_gzMatches && !_gz && !_bam) throw Exception("option -gz-matches belongs to -gz");
        if (_testFile && _bam) throw Exception("option -test-file compares text: not with -bam");
        if (!_inputInflate.empty() && _decompress) throw Exception("option -input-inflate belongs to -c");
        if (!_recordParse.empty() && _decompress) throw Exception("option -record-parse belongs to -c");
        if (_recordParseFasta && (_recordParse.empty() || !record_parse_on_device(_recordParse))) throw Exception("option -record-parse-fasta belongs to -record-parse device");
        if (_dictPieces && _decompress) throw Exception("option -dict-pieces belongs to -c: -d reads the pieces whenever the container holds them");
        if (_dictPieceAnchors && !_dictPieces) throw Exception("option -dict-piece-anchors belongs to -dict-pieces");
        if (_seqOnly) _noHeader = _noQual = true;             // "same as -noheader -noqual", /root/reference/README.md:56
        execute();
    } catch (const Exception&) {
        throw;
    } catch (const std::exception& e) {                        // bad_alloc and friends follow the EXCEPTION: contract too
        throw Exception(e.what());
    }
}

void Leon::execute() {
    if (_compress) executeCompression(); else executeDecompression();
}

// -test-file: "check decompressed file against original" (/root/reference/INSTALL:22): X.fastq.d against X.fastq (or X.fastq.gz) beside it
void Leon::testDecompressedFile() {
    std::string orig = _outputFilename.substr(0, _outputFilename.size() - (_gz ? 5 : 2));      // X.fastq.d or, under -gz, X.fastq.d.gz
    struct stat st_o, st_d;
    const bool plain = !_gz && ::stat(orig.c_str(), &st_o) == 0 && S_ISREG(st_o.st_mode);       // (-gz: read through gzread below)
    if (plain && ::stat(_outputFilename.c_str(), &st_d) == 0) {
        // both files are plain: compared in slices by all cores (pread at disjoint offsets); the first difference is the lowest one found
        int fa = ::open(orig.c_str(), O_RDONLY), fb = ::open(_outputFilename.c_str(), O_RDONLY);
        if (fa < 0 || fb < 0) { if (fa >= 0) ::close(fa); if (fb >= 0) ::close(fb); throw Exception("-test-file: cannot reopen the files"); }
        const uint64_t na = (uint64_t)st_o.st_size, nb = (uint64_t)st_d.st_size, n = std::min(na, nb);
        const uint32_t n_thr = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(_nbCores > 0 ? (uint64_t)_nbCores : usableCpus(), n / (64ull << 20) + 1));
        std::vector<uint64_t> first_diff(n_thr, ~0ull);
        std::vector<int> io_error(n_thr, 0);
        auto compare = [&](uint32_t t) {
            const uint64_t lo = n * t / n_thr, hi = n * (t + 1) / n_thr;
            std::vector<char> ba(4 << 20), bb(4 << 20);
            for (uint64_t at = lo; at < hi;) {
                const size_t want = (size_t)std::min<uint64_t>(ba.size(), hi - at);
                const ssize_t ga = ::pread(fa, ba.data(), want, (off_t)at), gb = ::pread(fb, bb.data(), want, (off_t)at);
                if (ga <= 0 || gb <= 0) { io_error[t] = 1; return; }
                const size_t m = (size_t)std::min(ga, gb);
                if (memcmp(ba.data(), bb.data(), m) != 0) {
                    size_t i = 0; while (ba[i] == bb[i]) i++;
                    first_diff[t] = at + i; return;
                }
                at += m;
            }
        };
        std::vector<std::thread> th;
        for (uint32_t t = 0; t < n_thr; t++) th.emplace_back(compare, t);
        for (auto& t : th) t.join();
        ::close(fa); ::close(fb);
        for (int e : io_error) if (e) throw Exception("-test-file: read error while comparing " + _outputFilename + " with " + orig);
        uint64_t at = ~0ull;
        for (uint64_t d : first_diff) at = std::min(at, d);
        if (at == ~0ull && na != nb) at = n;
        if (at != ~0ull) throw Exception("-test-file: " + _outputFilename + " differs from " + orig + " at byte " + std::to_string(at));
        std::cout << "test-file: " << _outputFilename << " is identical to " << orig << std::endl;
        return;
    }
    gzFile a = gzopen(orig.c_str(), "rb");
    if (!a) { orig += ".gz"; a = gzopen(orig.c_str(), "rb"); }
    if (!a) throw Exception("-test-file: the original file is not beside " + _outputFilename);
    gzFile b = gzopen(_outputFilename.c_str(), "rb");
    if (!b) { gzclose(a); throw Exception("-test-file: cannot reopen " + _outputFilename); }
    std::vector<char> ba(1 << 20), bb(1 << 20);
    uint64_t at = 0;
    bool same = true;
    for (;;) {
        const int na = gzread(a, ba.data(), (unsigned)ba.size()), nb = gzread(b, bb.data(), (unsigned)bb.size());
        if (na != nb || na < 0 || (na > 0 && memcmp(ba.data(), bb.data(), (size_t)na) != 0)) {
            same = false;
            for (int i = 0; i < std::min(na, nb) && ba[i] == bb[i]; i++) at++;
            break;
        }
        if (na == 0) break;
        at += (uint64_t)na;
    }
    gzclose(a); gzclose(b);
    if (!same) throw Exception("-test-file: " + _outputFilename + " differs from " + orig + " at byte " + std::to_string(at));
    std::cout << "test-file: " << _outputFilename << " is identical to " << orig << std::endl;
}

// ------------------------------------------------------------------------------------------------ self tests (no GPU)
int selftest_container(const std::string& path) {
    std::vector<uint8_t> a(100000), empty;
    for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)(i * 2654435761u >> 13);
    std::vector<uint64_t> t = { 1, 2, 3, ~0ull, 0 };
    {
        Container c(path, Container::CREATE);
        c.putBytes(Container::blockPath(GROUP_DNA, 0), a.data(), a.size());
        c.putBytes(Container::blockPath(GROUP_DNA, 1), empty.data(), 0);
        c.putBytes(Container::blockPath(GROUP_HEADER, 0), a.data(), 17);
        c.putBytes(DS_INFOBYTE, a.data(), 1);
        c.putU64(DS_DNA_TABLE, t.data(), t.size());
        c.putU64(DS_PARAMS, t.data(), 0);
        c.close();
    }
    Container c(path, Container::READ);
    bool ok = c.getBytes(Container::blockPath(GROUP_DNA, 0)) == a && c.getBytes(Container::blockPath(GROUP_DNA, 1)).empty() &&
              c.getBytes(Container::blockPath(GROUP_HEADER, 0)) == std::vector<uint8_t>(a.begin(), a.begin() + 17) && c.getU64(DS_DNA_TABLE) == t &&
              c.getU64(DS_PARAMS).empty() && c.exists(DS_INFOBYTE) && !c.exists(Container::blockPath(GROUP_QUAL, 0)) && !c.exists("nothing/here");
    bool threw = false;
    try { (void)c.getBytes("leon/dna/block_7"); } catch (const Exception&) { threw = true; }
    bool threw2 = false;
    try { (void)c.getBytes(DS_DNA_TABLE); } catch (const Exception&) { threw2 = true; }      // a u64 array is not a byte array
    ok = ok && threw && threw2;
    std::cout << (ok ? "container selftest OK" : "container selftest FAILED") << std::endl;
    return ok ? 0 : 1;
}

int selftest_bank(const std::string& path) {
    Bank bank(path);
    ReadBatch b;
    uint64_t n = 0, nb = 0, nh = 0, nq = 0, fnv_b = 1469598103934665603ull, fnv_h = fnv_b, fnv_q = fnv_b;
    auto mix = [](uint64_t& h, const std::string& s) { for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; } };
    const bool fq = bank.isFastq();
    for (;;) {
        b.clear();
        const uint64_t got = bank.next(b, 1000);
        if (!got) break;
        n += got; nb += b.bases.size(); nh += b.headers.size(); nq += b.quals.size();
        mix(fnv_b, b.bases); mix(fnv_h, b.headers); mix(fnv_q, b.quals);
    }
    std::cout << "{\"fastq\": " << (fq ? "true" : "false") << ", \"reads\": " << n << ", \"bases\": " << nb << ", \"header_bytes\": " << nh << ", \"qual_bytes\": " << nq
              << ", \"fasta_line_width\": " << bank.fastaLineWidth() << ", \"fnv_bases\": " << fnv_b << ", \"fnv_headers\": " << fnv_h << ", \"fnv_quals\": " << fnv_q;
    // the '+'-line table as the container stores it, read back the way -d reads it
    const std::string plus = bank.plusLines();
    const PlusLines L = PlusLines::decode(reinterpret_cast<const uint8_t*>(plus.data()), plus.size());
    uint64_t text_bytes = 0;
    for (const PlusLines::Exc& e : L.exc) text_bytes += e.text.size();
    std::cout << ", \"plus\": {\"bytes\": " << plus.size() << ", \"default\": " << (int)L.def << ", \"exceptions\": " << L.exc.size() << ", \"first_exception\": "
              << (L.exc.empty() ? -1ll : (long long)L.exc[0].read) << ", \"text_bytes\": " << text_bytes << "}}" << std::endl;
    return 0;
}

}  // namespace leon_host
