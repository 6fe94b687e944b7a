// ws_layout_check.cc -- WsLayout (my-slam_amd/csrc/ws_layout.h) by itself: mixed element types, counts of 0, 1, 7 and 8, an odd
// byte count, two binds.  Built stand-alone under AddressSanitizer and UBSan by tests/test_ws_layout_cxx.py; every part is written
// end to end inside a block of exactly bytes() bytes, so a part that reached past its end or past the block would be reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ws_layout.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

struct Fields {
    double *d8 = nullptr, *d1 = nullptr, *d0 = nullptr, *pair[2] = {nullptr, nullptr};
    float *f7 = nullptr, *f0 = nullptr;
    int32_t *i7 = nullptr, *i16 = nullptr;
    uint8_t *b7 = nullptr, *b0 = nullptr, *b1 = nullptr, *b65 = nullptr;
};
struct Want { uint8_t *const *field; size_t bytes; };       // a field read as bytes, and its part's size before rounding

static size_t round64(size_t b) { return (b + 63) & ~(size_t)63; }

int main()
{
    Fields f;
    WsLayout ws;
    CHECK(ws.bytes() == 0);
    ws.take(f.d8, 8);           // 64 bytes: exactly one line
    ws.take(f.f7, 7);           // 28
    ws.take(f.d0, 0);           // nothing: the next part's address
    ws.take(f.i7, 7);           // 28
    ws.take(f.b7, 7);           // an odd byte count
    ws.take(f.d1, 1);
    ws.take(f.pair[0], 7);      // fields of an array, as the double-buffered estimates are
    ws.take(f.pair[1], 7);
    ws.take(f.f0, 0);
    ws.take(f.b0, 0);           // two empty parts in a row
    ws.take(f.b1, 1);
    ws.take(f.b65, 65);         // one byte into a second line
    ws.take(f.i16, 16);         // 64 bytes again, the last part
    const Want want[] = {
        {(uint8_t *const *)&f.d8, 64}, {(uint8_t *const *)&f.f7, 28}, {(uint8_t *const *)&f.d0, 0}, {(uint8_t *const *)&f.i7, 28},
        {&f.b7, 7}, {(uint8_t *const *)&f.d1, 8}, {(uint8_t *const *)&f.pair[0], 56}, {(uint8_t *const *)&f.pair[1], 56},
        {(uint8_t *const *)&f.f0, 0}, {&f.b0, 0}, {&f.b1, 1}, {&f.b65, 65}, {(uint8_t *const *)&f.i16, 64},
    };
    const int n = (int)(sizeof want / sizeof want[0]);
    size_t sum = 0;
    for (int i = 0; i < n; i++) sum += round64(want[i].bytes);
    CHECK(ws.bytes() == sum);
    CHECK(ws.bytes() == 64 * 11);

    // the fields are read through memcpy: each is a pointer to its own type
    auto at = [&](int i) { uint8_t *p; memcpy(&p, want[i].field, sizeof p); return p; };
    std::vector<uint8_t> block[2] = {std::vector<uint8_t>(ws.bytes()), std::vector<uint8_t>(ws.bytes())};
    for (int round = 0; round < 2; round++) {
        uint8_t *base = block[round].data();
        ws.bind(base);
        size_t off = 0;
        for (int i = 0; i < n; i++) {
            const size_t o = (size_t)(at(i) - base);
            CHECK(at(i) >= base && o % 64 == 0);                        // base + k * 64
            CHECK(o == off);                                            // where the part before it ended: no overlap, no gap
            CHECK(o + want[i].bytes <= ws.bytes());                     // it ends inside the block
            if (i + 1 < n && want[i].bytes == 0) CHECK(at(i) == at(i + 1));
            off += round64(want[i].bytes);
        }
        CHECK(off == ws.bytes());
    }
    // after the second bind every field is in the second block, at the offset it had in the first
    ws.bind(block[0].data());
    std::vector<size_t> first;
    for (int i = 0; i < n; i++) first.push_back((size_t)(at(i) - block[0].data()));
    ws.bind(block[1].data());
    for (int i = 0; i < n; i++) CHECK(at(i) == block[1].data() + first[i]);

    // typed writes over every part, end to end, then a pattern check: a part that overlapped another would have been overwritten
    for (int i = 0; i < 8; i++) f.d8[i] = 1000.0 + i;
    for (int i = 0; i < 7; i++) { f.f7[i] = 2000.f + i; f.i7[i] = 3000 + i; f.b7[i] = (uint8_t)(40 + i); f.pair[0][i] = 5000.0 + i; f.pair[1][i] = 6000.0 + i; }
    f.d1[0] = 7000.0; f.b1[0] = 81;
    for (int i = 0; i < 65; i++) f.b65[i] = (uint8_t)(100 + i);
    for (int i = 0; i < 16; i++) f.i16[i] = 9000 + i;
    bool same = true;
    for (int i = 0; i < 8; i++) same = same && f.d8[i] == 1000.0 + i;
    for (int i = 0; i < 7; i++)
        same = same && f.f7[i] == 2000.f + i && f.i7[i] == 3000 + i && f.b7[i] == 40 + i && f.pair[0][i] == 5000.0 + i && f.pair[1][i] == 6000.0 + i;
    same = same && f.d1[0] == 7000.0 && f.b1[0] == 81;
    for (int i = 0; i < 65; i++) same = same && f.b65[i] == 100 + i;
    for (int i = 0; i < 16; i++) same = same && f.i16[i] == 9000 + i;
    CHECK(same);

    if (failures) return 1;
    printf("ws_layout_check ok: %d parts, %zu bytes\n", n, ws.bytes());
    return 0;
}
