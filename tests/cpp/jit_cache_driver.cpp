// CPU driver of the kernel cache's store (gaast_amd/csrc/device/jit_cache.cpp), built with -fsanitize=address,undefined by
// tests/test_jit_cache_cpu.py.  One check per sub-command, "OK" as the last line of a passing one:
//   sha | key | roundtrip <dir> | reject <dir> | baddirs <dir> | store <dir> <fill byte> <bytes> | verify <dir> <bytes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <string>
#include <vector>

#include <sys/stat.h>
#include <unistd.h>

#include "jit_cache.hpp"

using namespace gaast::jitcache;

#define CHECK(cond)                                                            \
    do {                                                                       \
        if (!(cond)) {                                                         \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            std::exit(1);                                                      \
        }                                                                      \
    } while (0)

static const std::string kRev = "0123456789ab";

static KeyFields fields() {
    KeyFields f;
    f.revision = kRev;
    f.compiler = "7.0";
    f.target = "gfx950";
    f.options = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"};
    f.entry = "gaast_jit";
    f.source = "extern \"C\" __global__ void gaast_jit() {}";
    return f;
}

static std::vector<char> random_bytes(size_t n, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<char> v(n);
    for (char& c : v) c = char(rng());
    return v;
}

static std::vector<char> read_file(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    CHECK(f.good());
    return std::vector<char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static void write_file(const std::string& path, const std::vector<char>& data, size_t n) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(data.data(), std::streamsize(n));
    CHECK(f.good());
}

// FIPS 180-4 example vectors (and the one-million 'a' message, fed in uneven pieces: the incremental path)
static void cmd_sha() {
    CHECK(hex(sha256("", 0)) == "e3b0c44298fc1c149afbf4c8996fb92427ae41e4649b934ca495991b7852b855");
    CHECK(hex(sha256("abc", 3)) == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad");
    const char* m448 = "abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq";
    CHECK(std::strlen(m448) * 8 == 448);
    CHECK(hex(sha256(m448, 56)) == "248d6a61d20638b8e5c026930c3e6039a33ce45964ff2167f6ecedd419db06c1");
    Sha256 s;
    const std::string a(1000000, 'a');
    for (size_t off = 0, step = 1; off < a.size(); off += step, step = step * 7 % 1009 + 1)
        s.update(a.data() + off, std::min(step, a.size() - off));
    CHECK(hex(s.finish()) == "cdc76e5c9914fb9281a1c7e284d73e67f1809a48a497200e046d39ccc7112cd0");
    // every message length around the padding boundaries agrees between one update and byte-wise updates
    for (size_t n = 0; n < 200; ++n) {
        Sha256 b;
        for (size_t i = 0; i < n; ++i) b.update(a.data() + i, 1);
        CHECK(b.finish() == sha256(a.data(), n));
    }
}

static void cmd_key() {
    const KeyFields base = fields();
    const Digest k0 = make_key(base);
    CHECK(make_key(fields()) == k0);
    std::vector<KeyFields> changed(8, base);
    changed[0].revision += "x";
    changed[1].compiler = "7.1";
    changed[2].target = "gfx942";
    changed[3].options[1] = "-O2";
    changed[4].options[2] = "-ffp-contract=fast";
    changed[5].options.push_back("-g");
    changed[6].entry = "gaast_chain";
    changed[7].source += " ";
    for (size_t i = 0; i < changed.size(); ++i) {
        CHECK(make_key(changed[i]) != k0);
        for (size_t j = 0; j < i; ++j) CHECK(make_key(changed[i]) != make_key(changed[j]));
    }
    // a byte moved between adjacent fields, for every adjacent pair
    KeyFields f;
    for (size_t i = 0; i + 1 < 8; ++i) {
        f = base;
        std::string* order[8] = {&f.revision, &f.compiler, &f.target, &f.options[0], &f.options[1], &f.options[2], &f.entry, &f.source};
        order[i + 1]->insert(order[i + 1]->begin(), order[i]->back());
        order[i]->pop_back();
        CHECK(make_key(f) != k0);
    }
    // the last option handed to the entry point's place: fewer options, same strings in the same order
    f = base;
    f.source = f.entry + f.source;
    f.entry = f.options.back();
    f.options.pop_back();
    CHECK(make_key(f) != k0);
}

static void cmd_roundtrip(const std::string& dir) {
    const size_t sizes[] = {0, 1, 115, 116, 4096, 70001, (1u << 20) + 12345};
    unsigned seed = 1;
    for (size_t n : sizes) {
        KeyFields f = fields();
        f.source += std::to_string(n);
        const Digest key = make_key(f);
        const std::vector<char> data = random_bytes(n, seed++);
        std::vector<char> back(3, 'x');
        CHECK(load(dir, kRev, key, &back) == Load::Missing && back.empty());
        CHECK(store(dir, kRev, key, data.data(), data.size()));
        CHECK(load(dir, kRev, key, &back) == Load::Ok);
        CHECK(back == data);
        const std::vector<char> file = read_file(file_path(dir, key));
        CHECK(file.size() == kHeaderBytes + n);
        CHECK(std::memcmp(file.data(), kMagic, 8) == 0);
        CHECK(std::memcmp(file.data() + kOffKey, key.data(), 32) == 0);
        CHECK(std::memcmp(file.data() + kOffRevision, kRev.data(), kRev.size()) == 0);
        // storing again replaces the file
        CHECK(store(dir, kRev, key, data.data(), data.size()));
        CHECK(load(dir, kRev, key, &back) == Load::Ok && back == data);
    }
    // a revision longer than its header field
    const std::string long_rev(40, 'r');
    const Digest key = make_key(fields());
    std::vector<char> back;
    CHECK(store(dir, long_rev, key, "xyz", 3));
    CHECK(load(dir, long_rev, key, &back) == Load::Ok && back == std::vector<char>({'x', 'y', 'z'}));
    CHECK(load(dir, kRev, key, &back) == Load::Rejected && back.empty());
}

static void cmd_reject(const std::string& dir) {
    const Digest key = make_key(fields());
    const std::string path = file_path(dir, key);
    const std::vector<char> data = random_bytes(5000, 42);
    std::vector<char> back;
    auto fresh = [&]() {
        CHECK(store(dir, kRev, key, data.data(), data.size()));
        CHECK(load(dir, kRev, key, &back) == Load::Ok && back == data);
        return read_file(path);
    };
    auto rejected_then_repaired = [&]() {
        back.assign(7, 'x');
        CHECK(load(dir, kRev, key, &back) == Load::Rejected);
        CHECK(back.empty());
        fresh();
    };
    const std::vector<char> good = fresh();
    // truncated at every header-field boundary, inside the header, in the middle and at the end of the payload
    const size_t cuts[] = {0, kOffVersion, kOffRevision, kOffKey, kOffLength, kOffHash, kHeaderBytes, 3, 50, 100,
                           kHeaderBytes + 1, kHeaderBytes + data.size() / 2, good.size() - 1};
    for (size_t cut : cuts) {
        write_file(path, good, cut);
        rejected_then_repaired();
    }
    // longer than its header says
    std::vector<char> longer = good;
    longer.push_back(0);
    write_file(path, longer, longer.size());
    rejected_then_repaired();
    // one flipped bit in each header field (the revision: in its text and in its padding; the length: low and high byte)
    // and in the payload
    const size_t flips[] = {kOffMagic, kOffMagic + 7, kOffVersion, kOffVersion + 3, kOffRevision, kOffRevision + 31, kOffKey, kOffKey + 31,
                            kOffLength, kOffLength + 7, kOffHash, kOffHash + 31, kHeaderBytes, kHeaderBytes + 2500, good.size() - 1};
    for (size_t at : flips)
        for (int bit : {0, 7}) {
            std::vector<char> bad = good;
            bad[at] = char(bad[at] ^ (1 << bit));
            write_file(path, bad, bad.size());
            rejected_then_repaired();
        }
    // a well-formed file of another revision under this name
    CHECK(store(dir, "ba9876543210", key, data.data(), data.size()));
    rejected_then_repaired();
    // ... and a well-formed file of another key under this name
    KeyFields other = fields();
    other.source += "//";
    CHECK(store(dir, kRev, make_key(other), data.data(), data.size()));
    CHECK(std::rename(file_path(dir, make_key(other)).c_str(), path.c_str()) == 0);
    rejected_then_repaired();
}

static void cmd_baddirs(const std::string& dir) {
    const Digest key = make_key(fields());
    std::vector<char> back;
    CHECK(!store(dir + "/missing", kRev, key, "abc", 3));
    CHECK(load(dir + "/missing", kRev, key, &back) == Load::Missing);
    CHECK(!store("", kRev, key, "abc", 3));
    // a regular file where the directory should be
    write_file(dir + "/plain", {'x'}, 1);
    CHECK(!store(dir + "/plain", kRev, key, "abc", 3));
    CHECK(!prepare_dir(dir + "/plain"));
    CHECK(!prepare_dir(dir + "/missing/deeper"));   // only the last component is created
    CHECK(prepare_dir(dir + "/made") && prepare_dir(dir + "/made"));
    CHECK(store(dir + "/made", kRev, key, "abc", 3));
    // read-only directory: the store fails and leaves nothing (root is not bound by the mode bits: then it may succeed)
    const std::string ro = dir + "/readonly";
    CHECK(::mkdir(ro.c_str(), 0555) == 0);
    const bool stored = store(ro, kRev, key, "abc", 3);
    if (::geteuid() != 0) {
        CHECK(!stored);
        CHECK(load(ro, kRev, key, &back) == Load::Missing);
    } else {
        std::printf("note: running as root, the read-only directory accepted the file\n");
    }
    ::chmod(ro.c_str(), 0755);
}

// concurrency: the payload is `bytes` copies of one fill byte, so that a file mixed from two writers cannot pass for either
static void cmd_store(const std::string& dir, int fill, size_t bytes) {
    const std::vector<char> data(bytes, char(fill));
    CHECK(store(dir, kRev, make_key(fields()), data.data(), data.size()));
}

static void cmd_verify(const std::string& dir, size_t bytes) {
    std::vector<char> back;
    CHECK(load(dir, kRev, make_key(fields()), &back) == Load::Ok);
    CHECK(back.size() == bytes);
    for (char c : back) CHECK(c == back[0]);
    std::printf("%s\n", (hex(make_key(fields())) + ".gaastco").c_str());
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    const std::string dir = argc > 2 ? argv[2] : "";
    if (cmd == "sha") cmd_sha();
    else if (cmd == "key") cmd_key();
    else if (cmd == "roundtrip" && argc == 3) cmd_roundtrip(dir);
    else if (cmd == "reject" && argc == 3) cmd_reject(dir);
    else if (cmd == "baddirs" && argc == 3) cmd_baddirs(dir);
    else if (cmd == "store" && argc == 5) cmd_store(dir, std::atoi(argv[3]), size_t(std::atol(argv[4])));
    else if (cmd == "verify" && argc == 4) cmd_verify(dir, size_t(std::atol(argv[3])));
    else {
        std::printf("usage: see the head of jit_cache_driver.cpp\n");
        return 2;
    }
    std::printf("OK\n");
    return 0;
}
