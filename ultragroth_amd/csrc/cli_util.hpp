// cli_util.hpp -- what the command-line tools of the setups share (main_dev_setup.cpp, main_zkey_new.cpp, main_ptau_prepare.cpp,
// main_zkey_verify.cpp): a number argument, a file written whole, the default device, and the option loop. Each tool keeps its
// own usage string, warnings, exit codes and output lines.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace ugcli {

// a decimal number in lo .. hi, the whole argument
inline bool numberArg(const char* s, long lo, long hi, long& out) {
    char* end = nullptr;
    const long v = strtol(s, &end, 10);
    if (!*s || *end || v < lo || v > hi) return false;
    out = v;
    return true;
}

inline void writeFile(const std::string& path, const void* data, size_t n) {
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)data, (std::streamsize)n);
    if (!f) throw std::runtime_error("cannot write " + path);
}

// ULTRAGROTH_DEVICE, else 0; -1 runs on host threads
inline long defaultDevice() {
    const char* e = getenv("ULTRAGROTH_DEVICE");
    return e ? atoi(e) : 0;
}

// One option of a tool's table. A flag takes no value; text takes any; a number must lie in lo .. hi (noSign: and must not start
// with '-'), otherwise `error` and the usage go to stderr.
struct Option {
    const char* name;
    bool* flag;
    std::string* text;
    long* number;
    long lo, hi;
    const char* error;
    bool noSign;
};
inline Option flagOption(const char* name, bool* v) { return {name, v, nullptr, nullptr, 0, 0, nullptr, false}; }
inline Option textOption(const char* name, std::string* v) { return {name, nullptr, v, nullptr, 0, 0, nullptr, false}; }
inline Option numberOption(const char* name, long* v, long lo, long hi, const char* error, bool noSign = false) {
    return {name, nullptr, nullptr, v, lo, hi, error, noSign};
}
inline Option validateOption(long* v, long lo, const char* error) { return numberOption("--validate", v, lo, 2, error); }
inline Option deviceOption(long* v) { return numberOption("--device", v, -1, 1024, "Error: --device takes a device number, or -1 for host threads\n"); }

// argv -> the options' targets and the positional arguments. false (after the usage on stderr): a number out of range, an unknown
// "--" argument, or an option whose value is missing.
inline bool parseArgs(int argc, char** argv, const std::vector<Option>& options, const char* usage, std::vector<std::string>& pos) {
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        const Option* o = nullptr;
        for (const Option& c : options)
            if (a == c.name && (c.flag || i + 1 < argc)) { o = &c; break; }
        if (o && o->flag) *o->flag = true;
        else if (o && o->text) *o->text = argv[++i];
        else if (o) {
            const char* v = argv[++i];
            if ((o->noSign && v[0] == '-') || !numberArg(v, o->lo, o->hi, *o->number)) { fputs(o->error, stderr); fputs(usage, stderr); return false; }
        }
        else if (a.rfind("--", 0) == 0) { fputs(usage, stderr); return false; }
        else pos.push_back(a);
    }
    return true;
}

}  // namespace ugcli
