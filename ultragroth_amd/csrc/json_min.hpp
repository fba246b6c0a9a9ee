// json_min.hpp -- the JSON the verifier's host code reads (verifier_api.cpp, verifier_records.cpp): a minimal parser and the
// decimal strings of snarkjs' files as field values.
#pragma once
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "pairing.hpp"

namespace ugv {
using namespace ug;
using namespace ug::pr;

// ---- minimal JSON (objects, arrays, strings, numbers, literals): what nlohmann::json::parse accepts of it --------------
struct JVal {
    enum Type { Null, Bool, Number, String, Array, Object } type = Null;
    std::string str;                       // String: the text; Number: its literal
    bool integral = false;
    std::vector<JVal> arr;
    std::vector<std::pair<std::string, JVal>> obj;
    const JVal& at(const char* key) const {
        if (type != Object) throw std::invalid_argument("not an object");
        const JVal* hit = nullptr;
        for (const auto& kv : obj) if (kv.first == key) hit = &kv.second;          // later duplicates win, as nlohmann
        if (!hit) throw std::invalid_argument("missing key");
        return *hit;
    }
    const JVal& at(size_t i) const {
        if (type != Array || i >= arr.size()) throw std::invalid_argument("not an array element");
        return arr[i];
    }
    const std::string& string() const {
        if (type != String) throw std::invalid_argument("not a string");
        return str;
    }
};
struct JParser {
    const char* p;
    explicit JParser(const char* s) : p(s) {}
    void ws() { while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r') p++; }
    [[noreturn]] void bad() { throw std::invalid_argument("malformed json"); }
    JVal parse_document() {
        JVal v = value(0);
        ws();
        if (*p) bad();
        return v;
    }
    JVal value(int depth) {
        if (depth > 64) bad();
        ws();
        JVal v;
        if (*p == '{') {
            v.type = JVal::Object; p++; ws();
            if (*p == '}') { p++; return v; }
            for (;;) {
                ws();
                if (*p != '"') bad();
                std::string key = string_literal();
                ws();
                if (*p != ':') bad();
                p++;
                v.obj.emplace_back(std::move(key), value(depth + 1));
                ws();
                if (*p == ',') { p++; continue; }
                if (*p == '}') { p++; return v; }
                bad();
            }
        }
        if (*p == '[') {
            v.type = JVal::Array; p++; ws();
            if (*p == ']') { p++; return v; }
            for (;;) {
                v.arr.push_back(value(depth + 1));
                ws();
                if (*p == ',') { p++; continue; }
                if (*p == ']') { p++; return v; }
                bad();
            }
        }
        if (*p == '"') { v.type = JVal::String; v.str = string_literal(); return v; }
        if (!strncmp(p, "true", 4)) { p += 4; v.type = JVal::Bool; return v; }
        if (!strncmp(p, "false", 5)) { p += 5; v.type = JVal::Bool; return v; }
        if (!strncmp(p, "null", 4)) { p += 4; return v; }
        if (*p == '-' || (*p >= '0' && *p <= '9')) {
            const char* s = p;
            if (*p == '-') p++;
            if (*p == '0') p++;
            else if (*p >= '1' && *p <= '9') while (*p >= '0' && *p <= '9') p++;
            else bad();
            v.integral = true;
            if (*p == '.') { v.integral = false; p++; if (*p < '0' || *p > '9') bad(); while (*p >= '0' && *p <= '9') p++; }
            if (*p == 'e' || *p == 'E') {
                v.integral = false; p++;
                if (*p == '+' || *p == '-') p++;
                if (*p < '0' || *p > '9') bad();
                while (*p >= '0' && *p <= '9') p++;
            }
            v.type = JVal::Number; v.str.assign(s, p);
            return v;
        }
        bad();
    }
    std::string string_literal() {
        std::string out;
        p++;                                                        // opening quote
        for (;;) {
            unsigned char ch = (unsigned char)*p;
            if (ch == 0 || ch < 0x20) bad();
            if (ch == '"') { p++; return out; }
            if (ch == '\\') {
                p++;
                switch (*p) {
                    case '"': out += '"'; break;   case '\\': out += '\\'; break; case '/': out += '/'; break;
                    case 'b': out += '\b'; break;  case 'f': out += '\f'; break;  case 'n': out += '\n'; break;
                    case 'r': out += '\r'; break;  case 't': out += '\t'; break;
                    case 'u': {
                        unsigned cp = 0;
                        for (int i = 1; i <= 4; i++) {
                            char h = p[i];
                            cp <<= 4;
                            if (h >= '0' && h <= '9') cp |= (unsigned)(h - '0');
                            else if (h >= 'a' && h <= 'f') cp |= (unsigned)(h - 'a' + 10);
                            else if (h >= 'A' && h <= 'F') cp |= (unsigned)(h - 'A' + 10);
                            else bad();
                        }
                        p += 4;
                        if (cp < 0x80) out += (char)cp;
                        else if (cp < 0x800) { out += (char)(0xc0 | (cp >> 6)); out += (char)(0x80 | (cp & 0x3f)); }
                        else { out += (char)(0xe0 | (cp >> 12)); out += (char)(0x80 | ((cp >> 6) & 0x3f)); out += (char)(0x80 | (cp & 0x3f)); }
                        break;
                    }
                    default: bad();
                }
                p++;
                continue;
            }
            out += (char)ch;
            p++;
        }
    }
};

// decimal string -> value mod q (E.f1.fromString); anything but digits is an error
inline F1 f1_from_decimal(const std::string& s) {
    if (s.empty()) throw std::invalid_argument("not a number");
    const F1 ten = f1_small(10);
    F1 acc = f1_zero();
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw std::invalid_argument("not a number");
        acc = acc * ten + f1_small((u32)(ch - '0'));
    }
    return acc;
}
// decimal string -> value mod r as a plain 256-bit integer (E.fr.fromString, then fromMontgomery in verify())
inline void fr_plain_from_decimal(u32 out[8], const std::string& s) {
    if (s.empty()) throw std::invalid_argument("not a number");
    u32 ten[8] = {10, 0, 0, 0, 0, 0, 0, 0};
    const Fr t = from_normal<FrParams>(ten);
    Fr acc = fp_zero<FrParams>();
    for (char ch : s) {
        if (ch < '0' || ch > '9') throw std::invalid_argument("not a number");
        u32 d[8] = {(u32)(ch - '0'), 0, 0, 0, 0, 0, 0, 0};
        acc = canon(add(canon(mul(acc, t)), from_normal<FrParams>(d)));
    }
    to_normal(out, acc);
}

}  // namespace ugv
