// The on-disk store of run-time compiled code objects (include/gaast_hip.h: "cache of compiled program kernels") and the key
// both cache levels share.  Plain C++17, no HIP: tests/cpp/jit_cache_driver.cpp compiles it under ASan / UBSan.
#pragma once

#include <array>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace gaast {
namespace jitcache {

using Digest = std::array<uint8_t, 32>;

// SHA-256 (FIPS 180-4), incremental
class Sha256 {
public:
    Sha256();
    void update(const void* data, size_t n);
    Digest finish();   // once

private:
    void block(const uint8_t* p);
    uint32_t h_[8];
    uint8_t buf_[64];
    size_t fill_ = 0;
    uint64_t bytes_ = 0;
};
Digest sha256(const void* data, size_t n);
std::string hex(const Digest& d);   // 64 lower-case digits

// Everything that decides the bytes hiprtc returns for one kernel
struct KeyFields {
    std::string revision;               // GAAST_KERNELS_REV: the generators (plan_fused.cpp, plan_chain_jit.cpp) and the launcher
    std::string compiler;               // hiprtcVersion, "major.minor"
    std::string target;                 // "gfx950"
    std::vector<std::string> options;   // as passed to hiprtcCompileProgram, in order
    std::string entry;                  // "gaast_jit" / "gaast_chain"
    std::string source;
};
// SHA-256 over: the format tag, revision, compiler, target, the number of options, every option, entry, source -- each one
// preceded by its length as a 64-bit little-endian integer (the number of options: that integer alone), so that no two
// different field lists give the same byte stream.
Digest make_key(const KeyFields& f);

// ---- the file: <dir>/<hex(key)>.gaastco, layout documented in include/gaast_hip.h ----------------------------------
constexpr char kMagic[8] = {'G', 'A', 'A', 'S', 'T', 'C', 'O', '\0'};
constexpr uint32_t kFormatVersion = 1;
constexpr size_t kRevisionBytes = 32;   // NUL-padded; a longer revision is cut (the key covers all of it)
constexpr size_t kOffMagic = 0, kOffVersion = 8, kOffRevision = 12, kOffKey = 44, kOffLength = 76, kOffHash = 84, kHeaderBytes = 116;

std::string file_path(const std::string& dir, const Digest& key);

// Writes <dir>/<key>.gaastco through a uniquely named temporary file in `dir` and rename(): whatever else writes the same
// name at the same time, a reader sees no file or one complete file.  False on any failure (nothing is thrown, no temporary
// file is left); `dir` is not created.
bool store(const std::string& dir, const std::string& revision, const Digest& key, const void* payload, size_t n) noexcept;

enum class Load { Missing, Rejected, Ok };
// Ok: *payload holds the code object, every header field and the payload's hash checked.  Rejected: a file is there and
// fails a check (magic, format version, revision, key, length against the file's size, hash of the payload) -- *payload is
// left empty.  Missing: no such file (or no permission to read it).
Load load(const std::string& dir, const std::string& revision, const Digest& key, std::vector<char>* payload) noexcept;

// gaast_hip_jit_cache_set_dir: the directory exists afterwards (its LAST component is created when missing, mode 0777 & ~umask)
bool prepare_dir(const std::string& path) noexcept;

}  // namespace jitcache
}  // namespace gaast
