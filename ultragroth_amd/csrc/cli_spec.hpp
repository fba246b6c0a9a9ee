// cli_spec.hpp -- the UltraGroth spec file of the command-line tools (main_dev_setup.cpp --ultra, main_zkey_new.cpp and
// main_zkey_verify.cpp built with -DUG_ULTRA): {"rand_indx": n, "round_signals": [...], "final_signals": [...]}, which signal
// carries the challenge and which private signals are committed before and after it.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>
#include "json_min.hpp"

namespace ugcli {

inline std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    return std::string((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
inline uint32_t numberOf(const ugv::JVal& v, const char* what) {
    if (v.type != ugv::JVal::Number || !v.integral || v.str.empty() || v.str[0] == '-') throw std::invalid_argument(std::string(what) + ": not an index");
    const unsigned long long x = strtoull(v.str.c_str(), nullptr, 10);
    if (x > 0xffffffffull) throw std::invalid_argument(std::string(what) + ": not an index");
    return (uint32_t)x;
}
inline std::vector<uint32_t> listOf(const ugv::JVal& v, const char* what) {
    if (v.type != ugv::JVal::Array) throw std::invalid_argument(std::string(what) + ": not a list");
    std::vector<uint32_t> out;
    for (const ugv::JVal& e : v.arr) out.push_back(numberOf(e, what));
    return out;
}

struct UltraSpec {
    uint32_t randIndx = 0;
    std::vector<uint32_t> roundSignals, finalSignals;
};
inline UltraSpec readUltraSpec(const std::string& path) {
    const std::string text = slurp(path);
    const ugv::JVal j = ugv::JParser(text.c_str()).parse_document();
    UltraSpec s;
    s.randIndx = numberOf(j.at("rand_indx"), "rand_indx");
    s.roundSignals = listOf(j.at("round_signals"), "round_signals");
    s.finalSignals = listOf(j.at("final_signals"), "final_signals");
    return s;
}

}  // namespace ugcli
