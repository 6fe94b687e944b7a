// orbv_workspace.cc -- host-only: the vocabulary handle's error text, destruction and staging growth (orbv_internal.h)
#include <cstdarg>
#include <cstdio>
#include <string>
#include "orbv_internal.h"

static thread_local std::string g_verr;
int vfail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_verr = buf;
    return code;
}
extern "C" const char *orbv_last_error(void) { return g_verr.c_str(); }

extern "C" void orbv_destroy(orbv_vocabulary *v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->stream) (void)hipStreamDestroy(v->stream);
    delete v;
}

int orbv_ensure_feat(orbv_vocabulary *v, size_t n)
{
    if (n <= v->cap_feat()) return ORBX_OK;
    VHIP(hipStreamSynchronize(v->stream));
    const size_t cap = n + n / 4 + 64;
    VTRY(v->d_feat.grow(cap * 32, vfail, "feature staging"));
    VTRY(v->d_out_i.grow(cap * 16, vfail, "transform results"));
    VTRY(v->h_pin.grow(cap * 48, vfail, "pinned feature staging"));
    return ORBX_OK;
}
