#include "jit_cache.hpp"

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstring>

#include <fcntl.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

namespace gaast {
namespace jitcache {

// ---- SHA-256 (FIPS 180-4, sections 4.1.2, 4.2.2, 5.3.3, 6.2) ----------------------------------------------------------
namespace {
constexpr uint32_t K[64] = {
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};

inline uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

void put_le(uint8_t* p, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) p[i] = uint8_t(v >> (8 * i));
}
uint64_t get_le(const uint8_t* p, int bytes) {
    uint64_t v = 0;
    for (int i = 0; i < bytes; ++i) v |= uint64_t(p[i]) << (8 * i);
    return v;
}
}  // namespace

Sha256::Sha256() : h_{0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19} {}

void Sha256::block(const uint8_t* p) {
    uint32_t w[64];
    for (int t = 0; t < 16; ++t) w[t] = uint32_t(p[4 * t]) << 24 | uint32_t(p[4 * t + 1]) << 16 | uint32_t(p[4 * t + 2]) << 8 | uint32_t(p[4 * t + 3]);
    for (int t = 16; t < 64; ++t) {
        const uint32_t s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
        const uint32_t s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
        w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    uint32_t a = h_[0], b = h_[1], c = h_[2], d = h_[3], e = h_[4], f = h_[5], g = h_[6], h = h_[7];
    for (int t = 0; t < 64; ++t) {
        const uint32_t t1 = h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
        const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h_[0] += a, h_[1] += b, h_[2] += c, h_[3] += d, h_[4] += e, h_[5] += f, h_[6] += g, h_[7] += h;
}

void Sha256::update(const void* data, size_t n) {
    const uint8_t* p = static_cast<const uint8_t*>(data);
    bytes_ += n;
    if (fill_) {
        const size_t take = n < 64 - fill_ ? n : 64 - fill_;
        std::memcpy(buf_ + fill_, p, take);
        fill_ += take, p += take, n -= take;
        if (fill_ < 64) return;
        block(buf_);
        fill_ = 0;
    }
    for (; n >= 64; p += 64, n -= 64) block(p);
    if (n) std::memcpy(buf_, p, n);
    fill_ = n;
}

Digest Sha256::finish() {
    const uint64_t bits = bytes_ * 8;
    uint8_t pad[72] = {0x80};
    const size_t npad = (fill_ < 56 ? 56 : 120) - fill_;
    for (int i = 0; i < 8; ++i) pad[npad + i] = uint8_t(bits >> (56 - 8 * i));
    update(pad, npad + 8);
    Digest d;
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 4; ++j) d[size_t(4 * i + j)] = uint8_t(h_[i] >> (24 - 8 * j));
    return d;
}

Digest sha256(const void* data, size_t n) {
    Sha256 s;
    s.update(data, n);
    return s.finish();
}

std::string hex(const Digest& d) {
    static const char digits[] = "0123456789abcdef";
    std::string s(64, '0');
    for (size_t i = 0; i < 32; ++i) s[2 * i] = digits[d[i] >> 4], s[2 * i + 1] = digits[d[i] & 15];
    return s;
}

// ---- key --------------------------------------------------------------------------------------------------------------
Digest make_key(const KeyFields& f) {
    Sha256 s;
    auto count = [&](uint64_t v) {
        uint8_t le[8];
        put_le(le, v, 8);
        s.update(le, 8);
    };
    auto field = [&](const std::string& v) {
        count(v.size());
        s.update(v.data(), v.size());
    };
    field("gaast-jit-cache-1");
    field(f.revision);
    field(f.compiler);
    field(f.target);
    count(f.options.size());
    for (const std::string& o : f.options) field(o);
    field(f.entry);
    field(f.source);
    return s.finish();
}

// ---- file -------------------------------------------------------------------------------------------------------------
std::string file_path(const std::string& dir, const Digest& key) { return dir + "/" + hex(key) + ".gaastco"; }

namespace {
// (hash: of the payload, or left zero -- load compares the fields before it only)
void make_header(uint8_t* h, const std::string& revision, const Digest& key, const void* payload, size_t n, bool hash) {
    std::memset(h, 0, kHeaderBytes);
    std::memcpy(h + kOffMagic, kMagic, sizeof(kMagic));
    put_le(h + kOffVersion, kFormatVersion, 4);
    std::memcpy(h + kOffRevision, revision.data(), revision.size() < kRevisionBytes ? revision.size() : kRevisionBytes);
    std::memcpy(h + kOffKey, key.data(), 32);
    put_le(h + kOffLength, n, 8);
    if (hash) {
        const Digest d = sha256(payload, n);
        std::memcpy(h + kOffHash, d.data(), 32);
    }
}

bool write_all(int fd, const void* data, size_t n) {
    const char* p = static_cast<const char*>(data);
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        p += w, n -= size_t(w);
    }
    return true;
}
}  // namespace

bool store(const std::string& dir, const std::string& revision, const Digest& key, const void* payload, size_t n) noexcept {
    try {
        if (dir.empty() || (!payload && n)) return false;
        static std::atomic<unsigned> serial{0};
        const std::string final_path = file_path(dir, key);
        // unique among the processes of this host (pid) and the calls of this process (serial); O_EXCL refuses a stale namesake
        const std::string tmp = final_path + ".tmp." + std::to_string(long(::getpid())) + "." + std::to_string(serial.fetch_add(1));
        const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_EXCL | O_CLOEXEC, 0666);
        if (fd < 0) return false;
        uint8_t header[kHeaderBytes];
        make_header(header, revision, key, payload, n, true);
        bool ok = write_all(fd, header, kHeaderBytes) && write_all(fd, payload, n);
        ok = (::close(fd) == 0) && ok;   // a full disk may only show at close
        ok = ok && ::rename(tmp.c_str(), final_path.c_str()) == 0;
        if (!ok) (void)::unlink(tmp.c_str());
        return ok;
    } catch (...) {
        return false;
    }
}

Load load(const std::string& dir, const std::string& revision, const Digest& key, std::vector<char>* payload) noexcept {
    try {
        payload->clear();
        if (dir.empty()) return Load::Missing;
        std::FILE* f = std::fopen(file_path(dir, key).c_str(), "rb");
        if (!f) return Load::Missing;
        struct Closer {
            std::FILE* f;
            ~Closer() { std::fclose(f); }
        } closer{f};
        struct stat st;
        if (::fstat(::fileno(f), &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < off_t(kHeaderBytes)) return Load::Rejected;
        uint8_t got[kHeaderBytes], want[kHeaderBytes];
        if (std::fread(got, 1, kHeaderBytes, f) != kHeaderBytes) return Load::Rejected;
        make_header(want, revision, key, nullptr, 0, false);
        // magic, format version, revision and key in one comparison: they are contiguous
        if (std::memcmp(got, want, kOffLength) != 0) return Load::Rejected;
        const uint64_t n = get_le(got + kOffLength, 8);
        if (n != uint64_t(st.st_size) - kHeaderBytes) return Load::Rejected;
        std::vector<char> data(static_cast<size_t>(n));
        if (n && std::fread(data.data(), 1, data.size(), f) != data.size()) return Load::Rejected;
        const Digest d = sha256(data.data(), data.size());
        if (std::memcmp(d.data(), got + kOffHash, 32) != 0) return Load::Rejected;
        payload->swap(data);
        return Load::Ok;
    } catch (...) {
        payload->clear();
        return Load::Rejected;
    }
}

bool prepare_dir(const std::string& path) noexcept {
    if (path.empty()) return false;
    if (::mkdir(path.c_str(), 0777) != 0 && errno != EEXIST) return false;
    struct stat st;
    return ::stat(path.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

}  // namespace jitcache
}  // namespace gaast
