// host_bgzf.h -- what the two forms of the BGZF inflate share (host_streams.cpp; inflate_kernels.hip for leon_bgzf_inflate_device), DESIGN.md 4.14
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace leon {

enum { BGZF_MEMBER = 0, BGZF_PARTIAL = 1, BGZF_FOREIGN = 2 };
int bgzf_header(const uint8_t* p, uint64_t avail, uint64_t* size, uint64_t* pay0);

// a member of the caller's table: where it begins, its raw deflate stream (absolute in the bytes), its first byte in the text, the
// trailer's two words; !ok: no BGZF member of its span, or an ISIZE above 65 536
struct BgzfMember { uint64_t at, pay0, text0, pay_size; uint32_t crc, isize; bool ok; };
int bgzf_prepare(const uint8_t* bytes, uint64_t n_bytes, const uint64_t* member_off, uint64_t n_members, const void* text, uint64_t text_cap,
                 uint64_t* n_text, std::vector<BgzfMember>& m, std::string& why);
std::string bgzf_refusal(uint64_t member, uint64_t at);

}  // namespace leon
