// The table of td_special_dev.h's SpecialTable, built on the host: a function of the allowed literals alone, shared by the handle
// (td_api_special.cpp uploads the result) and the CPU model (tests/twin/special_model.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "td_special_dev.h"

namespace td {

struct SpecialTableHost {
    std::vector<uint8_t> bytes;   // the literals, each dword-aligned and zero-padded to a multiple of 4 bytes (never empty)
    std::vector<uint32_t> off;    // [n + 1]
    std::vector<uint32_t> len;    // [n + 1]
    std::vector<int32_t> id;      // [n]
    std::vector<int32_t> parent;  // [n] the longest other literal that is a proper prefix of literal i, or -1
    std::vector<uint32_t> first2; // [SP_FIRST2_WORDS]
    uint32_t maxlen = 0;
};

// lits: non-empty literals with their ids, sorted bytewise (std::string compares as unsigned char), no string twice.
inline SpecialTableHost special_table_build(const std::vector<std::pair<std::string, int32_t>>& lits) {
    const size_t n = lits.size();
    SpecialTableHost T;
    T.off.assign(n + 1, 0);
    T.len.assign(n + 1, 0);
    T.first2.assign(SP_FIRST2_WORDS, 0);
    T.id.assign(n, 0);
    T.parent.assign(n, -1);
    for (size_t i = 0; i < n; ++i) {
        const std::string& x = lits[i].first;
        T.off[i] = (uint32_t)T.bytes.size();
        T.len[i] = (uint32_t)x.size();
        T.bytes.insert(T.bytes.end(), x.begin(), x.end());
        while (T.bytes.size() % 4) T.bytes.push_back(0);
        T.id[i] = lits[i].second;
        T.maxlen = std::max<uint32_t>(T.maxlen, (uint32_t)x.size());
        // longest proper prefix that is a literal: in sorted order a prefix stands in front of its extensions
        for (size_t j = i; j-- > 0;) {
            const std::string& y = lits[j].first;
            if (y.size() < x.size() && x.compare(0, y.size(), y) == 0) { T.parent[i] = (int32_t)j; break; }
            if (y.empty() || (uint8_t)y[0] != (uint8_t)x[0]) break;
        }
        const uint32_t b0 = (uint8_t)x[0];
        if (x.size() == 1) for (uint32_t b1 = 0; b1 < 256; ++b1) T.first2[(b0 << 8 | b1) >> 5] |= 1u << ((b0 << 8 | b1) & 31);
        else { const uint32_t kk = b0 << 8 | (uint8_t)x[1]; T.first2[kk >> 5] |= 1u << (kk & 31); }
    }
    if (T.bytes.empty()) T.bytes.push_back(0);
    return T;
}

}  // namespace td
