// ac_table.hh -- the pattern automaton of FCGPU_CLS_STRING, built on the host.
//
// Semantics: StringClassifier (elements/ids/stringclassifier.cc:94-101) runs
// AhoCorasick::match_first (ahocorasickplus.hh:113-123, ahocorasick.c:177-243,
// node.c:425-442) over the packet: the pattern at the earliest match end; of
// several patterns ending there, the longest (a final node reports its own
// pattern, else that of the nearest final node on its failure chain); -1
// without a match. Pattern lengths are 1..1024 (AC_PATTRN_MAX_LENGTH,
// actypes.h:165). A duplicate pattern is refused here; the reference drops it
// with a warning and then counts its no-match output one too high.
//
// Structure, one image:
//   cls[256]                 byte -> class: one class per distinct byte value
//                            of any pattern, class 0 for every other byte;
//   next[states][classes]    uint16 dense DFA, failure links resolved, state 0
//                            the root;
//   out[states - first_final] uint16, 1 + the id of the longest pattern ending
//                            at that state.
// States are numbered so that the final ones come last: a state s is final
// iff s >= first_final, so the scan tests a match with one compare and needs
// no bit in the entry (all 65535 states stay usable). The root is never final
// (no empty pattern). Every entry is written by the builder, so every index
// of a walk is in range for any text.
//
// No HIP here: the library (fcgpu_set_patterns), fcgpu_patterns_match and CPU
// programs share this file.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../../include/fastclick_gpu.h"

namespace fcac {

constexpr uint32_t kMaxPattern = 1024;            // AC_PATTRN_MAX_LENGTH
constexpr uint32_t kMaxStates = 65535;
constexpr size_t kMaxImage = (size_t)32 << 20;

struct Image {
    std::vector<uint8_t> bytes;   // cls, next, out; a multiple of 16 B
    uint32_t nstates = 1, nclasses = 1;
    uint32_t first_final = 1;     // states >= this are final
    uint32_t next_off = 256, out_off = 0;
    uint32_t lmax = 0;            // the longest pattern
    uint32_t npatterns = 0;
    const uint8_t *cls() const { return bytes.data(); }
    const uint16_t *next() const { return reinterpret_cast<const uint16_t *>(bytes.data() + next_off); }
    const uint16_t *out() const { return reinterpret_cast<const uint16_t *>(bytes.data() + out_off); }
};

// Build the image from n patterns concatenated in `bytes`. nports 0: ids are
// not bounded here (the submission checks npatterns). Returns FCGPU_OK or
// FCGPU_EINVAL with `err` set.
inline int build(const uint8_t *bytes, const uint32_t *lens, uint32_t n, uint32_t nports, Image &im, std::string &err) {
    im = Image{};
    if (n > kMaxStates) { err = "more than 65535 states"; return FCGPU_EINVAL; }
    if (nports && n > nports) {
        err = "pattern " + std::to_string(nports) + ": its output is not below nports";
        return FCGPU_EINVAL;
    }
    uint8_t cls[256] = {0};
    uint32_t ncls = 1;
    size_t total = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (lens[k] == 0) { err = "pattern " + std::to_string(k) + ": empty"; return FCGPU_EINVAL; }
        if (lens[k] > kMaxPattern) { err = "pattern " + std::to_string(k) + ": longer than 1024 bytes"; return FCGPU_EINVAL; }
        for (uint32_t j = 0; j < lens[k]; ++j)
            if (!cls[bytes[total + j]]) cls[bytes[total + j]] = 1;
        total += lens[k];
        im.lmax = std::max(im.lmax, lens[k]);
    }
    const uint32_t distinct = (uint32_t)std::count(cls, cls + 256, (uint8_t)1);
    // classes 1 .. distinct; with all 256 byte values in use there is no
    // "other" byte, and the classes are 0 .. 255
    for (uint32_t b = 0; b < 256; ++b)
        if (distinct == 256) cls[b] = (uint8_t)b;
        else if (cls[b]) cls[b] = (uint8_t)ncls++;
    if (distinct == 256) ncls = 256;
    // the trie: go[s * ncls + c] = child or 0 (the root is nobody's child)
    std::vector<uint32_t> go(ncls, 0), own(1, 0);   // own[s]: 1 + id of the pattern ending at s
    size_t at = 0;
    for (uint32_t k = 0; k < n; ++k) {
        uint32_t s = 0;
        for (uint32_t j = 0; j < lens[k]; ++j) {
            const uint32_t c = cls[bytes[at + j]];
            uint32_t t = go[(size_t)s * ncls + c];
            if (!t) {
                t = (uint32_t)own.size();
                if (t >= kMaxStates) { err = "more than 65535 states"; return FCGPU_EINVAL; }
                if (256 + ((size_t)t + 1) * (ncls + 1) * 2 + 32 > kMaxImage) {   // an upper bound of the image with t + 1 states
                    err = "automaton image above 32 MiB";
                    return FCGPU_EINVAL;
                }
                own.push_back(0);
                go.resize(go.size() + ncls, 0);
                go[(size_t)s * ncls + c] = t;
            }
            s = t;
        }
        if (own[s]) {
            err = "pattern " + std::to_string(k) + ": duplicate of pattern " + std::to_string(own[s] - 1);
            return FCGPU_EINVAL;
        }
        own[s] = k + 1;
        at += lens[k];
    }
    // breadth first: failure links, missing transitions filled from the
    // failure state's row, and each state's output (its own pattern, else its
    // failure state's: the nearest final node on the chain)
    const uint32_t ns = (uint32_t)own.size();
    std::vector<uint32_t> fail(ns, 0), order;
    order.reserve(ns);
    order.push_back(0);
    for (size_t q = 0; q < order.size(); ++q) {
        const uint32_t s = order[q];
        if (s && !own[s]) own[s] = own[fail[s]];
        for (uint32_t c = 0; c < ncls; ++c) {
            uint32_t &t = go[(size_t)s * ncls + c];
            const uint32_t via = s ? go[(size_t)fail[s] * ncls + c] : 0u;
            if (t) {
                fail[t] = via;
                order.push_back(t);
            } else {
                t = via;
            }
        }
    }
    // renumber: the states without an output first (the root stays 0), then the final ones
    std::vector<uint32_t> id(ns);
    uint32_t nf = 0;
    for (uint32_t s : order)
        if (!own[s]) id[s] = nf++;
    im.first_final = nf;
    for (uint32_t s : order)
        if (own[s]) id[s] = nf++;
    im.nstates = ns;
    im.nclasses = ncls;
    im.npatterns = n;
    im.next_off = 256;
    im.out_off = (uint32_t)((256 + (size_t)ns * ncls * 2 + 15) & ~(size_t)15);
    im.bytes.assign((im.out_off + (size_t)(ns - im.first_final) * 2 + 15) & ~(size_t)15, 0);
    memcpy(im.bytes.data(), cls, 256);
    uint16_t *nx = reinterpret_cast<uint16_t *>(im.bytes.data() + im.next_off);
    uint16_t *ou = reinterpret_cast<uint16_t *>(im.bytes.data() + im.out_off);
    for (uint32_t s = 0; s < ns; ++s) {
        for (uint32_t c = 0; c < ncls; ++c) nx[(size_t)id[s] * ncls + c] = (uint16_t)id[go[(size_t)s * ncls + c]];
        if (own[s]) ou[id[s] - im.first_final] = (uint16_t)own[s];
    }
    return FCGPU_OK;
}

// match_first over the image, as the device scans one chunk from the root:
// the id of the pattern reported at the first final state, or -1; *end (may
// be null) = the match's end position (bytes of text up to and including its
// last), 0 without a match.
inline int match_first(const Image &im, const uint8_t *text, uint32_t len, uint32_t *end) {
    const uint8_t *cls = im.cls();
    const uint16_t *next = im.next();
    uint32_t s = 0;
    if (end) *end = 0;
    for (uint32_t p = 0; p < len; ++p) {
        s = next[(size_t)s * im.nclasses + cls[text[p]]];
        if (s >= im.first_final) {
            if (end) *end = p + 1;
            return (int)im.out()[s - im.first_final] - 1;
        }
    }
    return -1;
}

}  // namespace fcac
