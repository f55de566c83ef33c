// host_plan_check.cpp -- leon_amd/host/leon_plan.hpp (the arithmetic of `leon -d` that needs no device) against brute-force models
// written here: records formatted byte by byte, letter tables painted base by base, tables damaged one word at a time.
// Stand-alone: g++ -std=c++17 tests/host_plan_check.cpp, nothing to link; tests/test_host_plan_cpu.py builds it plain and under
// AddressSanitizer + UBSan.
#include "../leon_amd/host/leon_plan.hpp"

#include <cstdio>
#include <functional>

using namespace leon_host;
using namespace leon_host::layout;

static int g_checks = 0;
#define REQUIRE(cond) do { g_checks++; if (!(cond)) { fprintf(stderr, "host_plan_check: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// ---------------------------------------------------------------------------------------------- record length
// the record as `-d` writes it, one byte after the other
static std::string format_record(bool fastq, bool has_header, const std::string& header, uint64_t read_index, const std::string& seq, uint64_t wrap, int plus_kind,
                                 const std::string& plus_text) {
    std::string t;
    t.push_back(fastq ? '@' : '>');
    const std::string name = has_header ? header : std::to_string(read_index);
    for (char c : name) t.push_back(c);
    t.push_back('\n');
    if (wrap && seq.size() > wrap) {
        for (size_t i = 0; i < seq.size(); i++) { t.push_back(seq[i]); if ((i + 1) % wrap == 0 || i + 1 == seq.size()) t.push_back('\n'); }
    } else { for (char c : seq) t.push_back(c); t.push_back('\n'); }
    if (fastq) {
        t.push_back('+');
        if (plus_kind == 1) for (char c : name) t.push_back(c);
        if (plus_kind == 2) for (char c : plus_text) t.push_back(c);
        t.push_back('\n');
        for (size_t i = 0; i < seq.size(); i++) t.push_back('I');
        t.push_back('\n');
    }
    return t;
}

static int check_record_lengths() {
    const std::string header = "read/1 some text", plus_text = "own";
    const uint64_t lens[] = {0, 1, 61}, indices[] = {9, 10, 99, 100};
    for (int fastq = 0; fastq < 2; fastq++)
        for (int has_header = 0; has_header < 2; has_header++)
            for (uint64_t idx : indices)
                for (uint64_t len : lens) {
                    const uint64_t wraps[] = {0, 1, len - 1, len, len + 1};           // (len 0: len - 1 is a width no sequence reaches)
                    for (uint64_t wrap : wraps)
                        for (int kind = 0; kind < 3; kind++) {
                            const std::string seq(len, 'A');
                            const std::string want = format_record(fastq, has_header, header, idx, seq, wrap, kind, plus_text);
                            const uint64_t hl = has_header ? header.size() : plan::index_text_len(idx);
                            const uint64_t extra = fastq ? plan::plus_extra_len((uint8_t)kind, hl, plus_text.size()) : 0;
                            REQUIRE(plan::record_text_len(hl, len, wrap, fastq, extra) == want.size());
                            // the closed form over many records of one '+' kind is the sum of its records
                            if (kind < 2) REQUIRE(plan::records_text_len(3, 3 * hl, 3 * plan::seq_text_len(len, wrap), 3 * len, fastq, (uint8_t)kind) == 3 * want.size());
                        }
                }
    return 0;
}

// ---------------------------------------------------------------------------------------------- letter clipping
struct Letters { std::vector<uint64_t> runs, pos; std::vector<uint8_t> bytes; };
// base by base: is it in a run, and which odd byte (0: none) lies on it
static void paint(const std::vector<uint64_t>& runs, const std::vector<uint64_t>& pos, const uint8_t* bytes, uint64_t at, std::vector<uint8_t>& lower, std::vector<uint8_t>& odd) {
    for (size_t r = 0; r < runs.size(); r += 2) for (uint64_t i = runs[r]; i < runs[r + 1]; i++) lower[at + i] = 1;
    for (size_t i = 0; i < pos.size(); i++) odd[at + pos[i]] = bytes[i];
}
static int check_clipping(const Letters& L, const std::vector<uint64_t>& joins) {
    const uint64_t n = joins.back();
    std::vector<uint8_t> want_lower(n, 0), want_odd(n, 0), got_lower(n, 0), got_odd(n, 0);
    paint(L.runs, L.pos, L.bytes.data(), 0, want_lower, want_odd);
    for (size_t j = 0; j + 1 < joins.size(); j++) {
        const uint64_t b0 = joins[j], b1 = joins[j + 1];
        const plan::LetterSlice s = plan::clip_letters(L.runs, L.pos, b0, b1);
        REQUIRE(s.runs.size() % 2 == 0 && s.first_pos + s.pos.size() <= L.pos.size());
        for (size_t r = 0; r < s.runs.size(); r += 2) {
            REQUIRE(s.runs[r] < s.runs[r + 1] && s.runs[r + 1] <= b1 - b0);              // never empty, never outside the round
            if (r) REQUIRE(s.runs[r - 1] <= s.runs[r]);
        }
        for (size_t i = 0; i < s.pos.size(); i++) REQUIRE(s.pos[i] < b1 - b0);
        // what the model says lies in [b0, b1)
        uint64_t want_runs = 0, want_pos = 0;
        for (size_t r = 0; r < L.runs.size(); r += 2) want_runs += L.runs[r] < b1 && L.runs[r + 1] > b0;
        for (uint64_t p : L.pos) want_pos += p >= b0 && p < b1;
        REQUIRE(s.runs.size() / 2 == want_runs && s.pos.size() == want_pos);
        paint(s.runs, s.pos, L.bytes.data() + s.first_pos, b0, got_lower, got_odd);
    }
    REQUIRE(got_lower == want_lower && got_odd == want_odd);     // the rounds' shares together are the whole table
    return 0;
}
static int check_letter_clipping() {
    // rounds [0,100) [100,200) [200,300) [300,400): a run across the join at 100, one that ends exactly at 200, one that begins exactly
    // at 200, positions at 200 (a round's first base) and 299 (its last), nothing at all in [300,400)
    Letters L;
    L.runs = {90, 110, 150, 200, 200, 230};
    L.pos = {5, 200, 250, 299};
    L.bytes = {'R', 'Y', 'K', 'M'};
    const std::vector<uint64_t> joins = {0, 100, 200, 300, 400};
    if (check_clipping(L, joins)) return 1;
    const plan::LetterSlice empty = plan::clip_letters(L.runs, L.pos, 300, 400);
    REQUIRE(empty.runs.empty() && empty.pos.empty());
    const plan::LetterSlice second = plan::clip_letters(L.runs, L.pos, 100, 200);
    REQUIRE((second.runs == std::vector<uint64_t>{0, 10, 50, 100}) && second.pos.empty());
    const plan::LetterSlice third = plan::clip_letters(L.runs, L.pos, 200, 300);
    REQUIRE((third.runs == std::vector<uint64_t>{0, 30}) && (third.pos == std::vector<uint64_t>{0, 50, 99}) && third.first_pos == 1);
    // the same table cut at other places: one round, rounds of one base around a join, a run that covers whole rounds
    if (check_clipping(L, {0, 400})) return 1;
    if (check_clipping(L, {0, 99, 100, 101, 199, 200, 201, 400})) return 1;
    Letters wide;
    wide.runs = {0, 400};
    if (check_clipping(wide, joins)) return 1;
    return check_clipping(Letters(), joins);
}

// ---------------------------------------------------------------------------------------------- validators
static bool throws(const std::function<void()>& f, const char* with) {
    try { f(); } catch (const Exception& e) { return std::string(e.what()).find(with) != std::string::npos; }
    return false;
}
static bool passes(const std::function<void()>& f) {
    try { f(); } catch (const Exception& e) { fprintf(stderr, "host_plan_check: refused: %s\n", e.what()); return false; }
    return true;
}

static int check_validators() {
    const std::string file = "x.leon";
    // three read blocks of 4 reads, the last one partial: 10 reads, 100 bases
    std::vector<uint64_t> params(PARAM_COUNT, 0);
    params[P_VERSION_MAJOR] = 1; params[P_KMER_SIZE] = 31; params[P_READS_PER_BLOCK] = 4; params[P_N_READS] = 10; params[P_N_ANCHORS] = 5;
    params[P_BLOOM_TAI] = 1000; params[P_BLOOM_N_HASH] = 7; params[P_BLOOM_BLOCK_NBITS] = 12; params[P_TOTAL_BASES] = 100; params[P_CONTAINER_REV] = CONTAINER_REV;
    const std::vector<uint8_t> info = {0};
    plan::Params p;
    REQUIRE(passes([&] { p = plan::check_params(file, info, params); }));
    REQUIRE(p.n_blocks == 3 && p.k == 31 && p.rpb == 4 && p.n_reads == 10 && p.total_bases == 100 && p.rev == CONTAINER_REV);
    // implausible parameters, one word at a time
    const struct { uint32_t word; uint64_t value; } implausible[] = {
        {P_KMER_SIZE, 2}, {P_KMER_SIZE, 64}, {P_READS_PER_BLOCK, 0}, {P_READS_PER_BLOCK, (1ull << 30) + 1}, {P_BLOOM_N_HASH, 0}, {P_BLOOM_N_HASH, 11},
        {P_BLOOM_BLOCK_NBITS, 3}, {P_BLOOM_BLOCK_NBITS, 17}, {P_N_ANCHORS, (1ull << 32) + 1}, {P_N_READS, (1ull << 40) + 1}, {P_TOTAL_BASES, (1ull << 46) + 1}};
    for (const auto& w : implausible) {
        std::vector<uint64_t> bad = params;
        bad[w.word] = w.value;
        REQUIRE(throws([&] { plan::check_params(file, info, bad); }, "x.leon: implausible parameters in the metadata"));
    }
    {
        std::vector<uint64_t> bad = params;
        bad[P_VERSION_MAJOR] = 2;
        REQUIRE(throws([&] { plan::check_params(file, info, bad); }, "x.leon was written by an incompatible version"));
        bad = params; bad[P_CONTAINER_REV] = CONTAINER_REV + 1;
        REQUIRE(throws([&] { plan::check_params(file, info, bad); }, "was written by a later build (container revision 3, this build reads up to 2)"));
        bad = params; bad.resize(PARAM_COUNT_REV1 - 1);
        REQUIRE(throws([&] { plan::check_params(file, info, bad); }, "x.leon: metadata is not what this build writes"));
        REQUIRE(throws([&] { plan::check_params(file, std::vector<uint8_t>(), params); }, "metadata is not what this build writes"));
        bad = params; bad.resize(PARAM_COUNT_REV1);                                  // a file of revision 1 has no revision word
        REQUIRE(passes([&] { p = plan::check_params(file, info, bad); }) && p.rev == 1);
        p = plan::check_params(file, info, params);
    }
    // block tables: payload bytes, reads, bases (text bytes for the headers)
    const std::vector<uint64_t> tdna = {50, 4, 40, 60, 4, 40, 30, 2, 20};
    REQUIRE(passes([&] { plan::check_dna_table(file, tdna, p); }));
    const struct { size_t word; uint64_t value; } dna_damage[] = {{1, 5}, {1, 3}, {2, 41}, {2, 101}, {8, 19}, {7, 3}, {2, ~0ull}};
    for (const auto& d : dna_damage) {
        std::vector<uint64_t> bad = tdna;
        bad[d.word] = d.value;
        REQUIRE(throws([&] { plan::check_dna_table(file, bad, p); }, "x.leon: the DNA block table does not add up"));
    }
    REQUIRE(throws([&] { plan::check_dna_table(file, std::vector<uint64_t>(tdna.begin(), tdna.end() - 3), p); }, "the DNA block table does not match the read count"));
    std::vector<uint64_t> thdr = {20, 4, 80, 21, 4, 81, 12, 2, 40};
    REQUIRE(passes([&] { plan::check_header_table(file, thdr, tdna, p); }) && thdr.size() == 9);
    {
        std::vector<uint64_t> bad = thdr;
        bad[4] = 3;
        REQUIRE(throws([&] { plan::check_header_table(file, bad, tdna, p); }, "x.leon: header and DNA blocks disagree"));
        bad = thdr; bad[5] = (1ull << 40) + 1;
        REQUIRE(throws([&] { plan::check_header_table(file, bad, tdna, p); }, "the header block table does not add up"));
        bad = thdr; bad.pop_back();
        REQUIRE(throws([&] { plan::check_header_table(file, bad, tdna, p); }, "the header block table does not match the read count"));
        // two words per block: a table of revision 1 is widened (64 bytes of text per header to begin with), a later one refused
        std::vector<uint64_t> two = {20, 4, 21, 4, 12, 2};
        REQUIRE(throws([&] { plan::check_header_table(file, two, tdna, p); }, "the header block table does not match the read count"));
        plan::Params p1 = p;
        p1.rev = 1;
        REQUIRE(passes([&] { plan::check_header_table(file, two, tdna, p1); }) && (two == std::vector<uint64_t>{20, 4, 256, 21, 4, 256, 12, 2, 128}));
    }
    const std::vector<uint64_t> tqual = {33, 4, 40, 34, 4, 40, 20, 2, 20};
    REQUIRE(passes([&] { plan::check_qual_table(file, tqual, tdna, p); }));
    for (size_t word : {1, 5}) {
        std::vector<uint64_t> bad = tqual;
        bad[word]++;
        REQUIRE(throws([&] { plan::check_qual_table(file, bad, tdna, p); }, "x.leon: quality and DNA blocks disagree"));
    }
    REQUIRE(throws([&] { plan::check_qual_table(file, std::vector<uint64_t>(8, 0), tdna, p); }, "the quality block table does not match the read count"));
    // the checksum table: the kind, then three words per block
    std::vector<uint64_t> tsum(1 + 3 * 3, 0x1234);
    tsum[0] = CHECKSUM_CRC32;
    REQUIRE(passes([&] { plan::check_checksum_table(file, tsum, 3); }));
    {
        std::vector<uint64_t> bad = tsum;
        bad[0] = 7;
        REQUIRE(throws([&] { plan::check_checksum_table(file, bad, 3); }, "x.leon: unknown checksum kind 7 in leon/metadata/checksums (this build knows 1 = CRC-32)"));
        bad = tsum; bad.pop_back();
        REQUIRE(throws([&] { plan::check_checksum_table(file, bad, 3); }, "the checksum table does not match the read count"));
        REQUIRE(throws([&] { plan::check_checksum_table(file, tsum, 4); }, "the checksum table does not match the read count"));
        REQUIRE(throws([&] { plan::check_checksum_table(file, std::vector<uint64_t>(), 0); }, "the checksum table does not match the read count"));
    }
    // the letter tables
    const std::vector<uint64_t> stored_runs = {LETTERS_RUNS_AND_BYTES, 10, 20, 20, 30, 90, 100};
    std::vector<uint64_t> runs = stored_runs;
    REQUIRE(passes([&] { plan::check_letter_runs(runs, 100); }) && (runs == std::vector<uint64_t>(stored_runs.begin() + 1, stored_runs.end())));
    const struct { size_t word; uint64_t value; const char* what; } run_damage[] = {
        {3, 19, "letters: leon/metadata/letter_runs run 1 overlaps the run before it"},      // run 1 begins inside run 0
        {0, 2, "letters: leon/metadata/letter_runs is of unknown kind 2 (this build knows 1)"},
        {2, 10, "letter_runs run 0 is empty or runs backwards"}, {4, 19, "letter_runs run 1 is empty or runs backwards"},
        {6, 101, "letter_runs run 2 ends behind the file's 100 bases"}};
    for (const auto& d : run_damage) {
        std::vector<uint64_t> bad = stored_runs;
        bad[d.word] = d.value;
        REQUIRE(throws([&] { plan::check_letter_runs(bad, 100); }, d.what));
    }
    {
        std::vector<uint64_t> bad = stored_runs;
        bad.pop_back();
        REQUIRE(throws([&] { plan::check_letter_runs(bad, 100); }, "letter_runs does not hold pairs"));
        bad.clear();
        REQUIRE(throws([&] { plan::check_letter_runs(bad, 100); }, "letters: leon/metadata/letter_runs is empty"));
    }
    const std::vector<uint64_t> pos = {0, 50, 99};
    const std::vector<uint8_t> bytes = {'R', 'Y', 'K'};
    REQUIRE(passes([&] { plan::check_letter_bytes(pos, bytes, 100); }));
    REQUIRE(passes([&] { plan::check_letter_bytes(std::vector<uint64_t>(), std::vector<uint8_t>(), 100); }));
    REQUIRE(throws([&] { plan::check_letter_bytes({0, 50, 100}, bytes, 100); }, "letters: leon/metadata/letter_odd_pos position 2 lies behind the file's 100 bases"));
    REQUIRE(throws([&] { plan::check_letter_bytes({0, 50, 50}, bytes, 100); }, "letter_odd_pos position 2 is not behind the one before it"));
    REQUIRE(throws([&] { plan::check_letter_bytes({0, 50}, bytes, 100); }, "letters: leon/metadata/letter_odd_bytes holds 3 bytes for 2 positions"));
    return 0;
}

int main() {
    if (check_record_lengths() || check_letter_clipping() || check_validators()) return 1;
    // prefix sums, with and without a stride
    const uint64_t sizes[] = {3, 9, 0, 9, 5, 9};
    if (plan::prefix_sums(sizes, 6) != std::vector<uint64_t>{0, 3, 12, 12, 21, 26, 35} || plan::prefix_sums(sizes, 3, 2) != std::vector<uint64_t>{0, 3, 3, 8} ||
        plan::prefix_sums(sizes, 0) != std::vector<uint64_t>{0}) { fprintf(stderr, "host_plan_check: prefix_sums\n"); return 1; }
    printf("host_plan_check: ok, %d checks\n", g_checks);
    return 0;
}
