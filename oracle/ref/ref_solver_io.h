/*
 * ref_solver_io.h -- what the three solver drivers (ref_sim3.cc, ref_pnp.cc, ref_init.cc) share: the record file format of their
 * requests and responses, and the scripted uniform source.  TEST INFRASTRUCTURE ONLY.  tests/ref_solvers.py is the other end.
 *
 * A file is a sequence of records, all little-endian:
 *     char  tag[8]      the name, NUL padded
 *     int32 dtype       0 uint8, 1 int32, 2 float32, 3 float64
 *     int32 rows, cols  the payload is rows * cols values, row-major
 *     payload
 * A request holds each tag once; the driver looks records up by name.  A response is ordered: a driver writes the records of one
 * call (or set, or motion) in a fixed order and repeats the group, so the k-th record of a tag belongs to the k-th group.
 *
 * The scripted source is tests/sim3_cases.py's Lcg: state = (seed * 2654435761 + 12345) mod 2^31, then
 * state = (1103515245 * state + 12345) mod 2^31 per value, values in [0, 2^31 - 1] = glibc's RAND_MAX.  Each driver defines
 * rand() as this source and srand() as a counter that changes nothing, so DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/
 * Random.cpp:47, linked unmodified) draws from the script, and the library under test is given the same source.
 */
#ifndef REF_SOLVER_IO_H
#define REF_SOLVER_IO_H

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

static_assert(RAND_MAX == 2147483647, "the scripted source has glibc's RAND_MAX");

namespace refio {

enum { U8 = 0, I32 = 1, F32 = 2, F64 = 3 };
static const int kSize[4] = {1, 4, 4, 8};

static const char *g_name = "ref";
[[noreturn]] inline void refuse(const char *m)
{
    std::fprintf(stderr, "%s: %s\n", g_name, m);
    std::exit(2);
}

struct Record {
    int dtype, rows, cols;
    std::vector<unsigned char> bytes;
    size_t count() const { return (size_t)rows * cols; }
    template <typename T> const T *as(int want) const
    {
        if (dtype != want) refuse("a request record has the wrong type");
        return (const T *)bytes.data();
    }
};

class Request {
public:
    explicit Request(const char *path)
    {
        FILE *f = std::fopen(path, "rb");
        if (!f) refuse("cannot open the request");
        for (;;) {
            char tag[8];
            int32_t head[3];
            if (std::fread(tag, 1, 8, f) != 8) break;
            if (std::fread(head, 4, 3, f) != 3) refuse("truncated request");
            if (head[0] < 0 || head[0] > 3 || head[1] < 0 || head[2] < 0 || (int64_t)head[1] * head[2] > (1 << 26)) refuse("bad record header");
            Record r;
            r.dtype = head[0];
            r.rows = head[1];
            r.cols = head[2];
            r.bytes.resize(r.count() * kSize[r.dtype] + 8);        /* never empty: data() is a valid pointer */
            size_t n = r.count() * kSize[r.dtype];
            if (n && std::fread(r.bytes.data(), 1, n, f) != n) refuse("truncated request");
            std::string name(tag, strnlen(tag, 8));
            if (recs_.count(name)) refuse("a request tag given twice");
            recs_[name] = r;
        }
        std::fclose(f);
    }
    const Record &get(const char *tag) const
    {
        std::map<std::string, Record>::const_iterator it = recs_.find(tag);
        if (it == recs_.end()) {
            std::fprintf(stderr, "%s: the request lacks '%s'\n", g_name, tag);
            std::exit(2);
        }
        return it->second;
    }
    bool has(const char *tag) const { return recs_.count(tag) != 0; }
    const Record &get(const char *tag, int dtype, int rows, int cols) const
    {
        const Record &r = get(tag);
        if (r.dtype != dtype || (rows >= 0 && r.rows != rows) || (cols >= 0 && r.cols != cols)) {
            std::fprintf(stderr, "%s: request record '%s' has the wrong type or shape\n", g_name, tag);
            std::exit(2);
        }
        return r;
    }

private:
    std::map<std::string, Record> recs_;
};

class Response {
public:
    explicit Response(const char *path) : f_(std::fopen(path, "wb"))
    {
        if (!f_) refuse("cannot open the response");
    }
    void put(const char *tag, int dtype, int rows, int cols, const void *data)
    {
        char t[8] = {0};
        std::strncpy(t, tag, 8);
        int32_t head[3] = {dtype, rows, cols};
        size_t n = (size_t)rows * cols * kSize[dtype];
        if (std::fwrite(t, 1, 8, f_) != 8 || std::fwrite(head, 4, 3, f_) != 3 || (n && std::fwrite(data, 1, n, f_) != n)) refuse("write failed");
    }
    void i32(const char *tag, int v) { int32_t x = v; put(tag, I32, 1, 1, &x); }
    void f32(const char *tag, float v) { put(tag, F32, 1, 1, &v); }
    void flags(const char *tag, const std::vector<bool> &v)
    {
        std::vector<unsigned char> b(v.size() + 1);
        for (size_t i = 0; i < v.size(); i++) b[i] = v[i] ? 1 : 0;
        put(tag, U8, 1, (int)v.size(), b.data());
    }
    void close()
    {
        if (std::fclose(f_) != 0) refuse("write failed");
        f_ = 0;
    }

private:
    FILE *f_;
};

/* the scripted source */
static uint32_t g_lcg = 0;
static int g_rand_calls = 0, g_srand_calls = 0;
inline void lcg_seed(int64_t seed) { g_lcg = (uint32_t)(((uint64_t)seed * 2654435761ull + 12345ull) % 2147483648ull); }
inline int lcg_next()
{
    g_lcg = (uint32_t)((1103515245ull * (uint64_t)g_lcg + 12345ull) % 2147483648ull);
    return (int)g_lcg;
}

} // namespace refio

/* replaces libc's in the driver: the only caller is DUtils::Random */
extern "C" int rand(void) noexcept
{
    refio::g_rand_calls++;
    return refio::lcg_next();
}
extern "C" void srand(unsigned int) noexcept { refio::g_srand_calls++; }

#endif
