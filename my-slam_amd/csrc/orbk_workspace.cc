// orbk_workspace.cc -- host-only: the keyframe database handle's error text, life and the growth of its device memory
#include <cstdarg>
#include <cstdio>
#include <string>
#include "orbk_internal.h"
#include "../../include/orbv.h"

static thread_local std::string g_kerr;
int kfail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_kerr = buf;
    return code;
}
extern "C" const char *orbk_last_error(void) { return g_kerr.c_str(); }

int orbk_ensure_io(orbk_database *db, size_t bytes)
{
    if (bytes <= db->cap_io()) return ORBX_OK;
    KHIP(hipStreamSynchronize(db->stream));
    const size_t cap = align16(bytes + bytes / 2);
    KTRY(db->d_io.grow(cap, kfail, "query I/O block"));
    KTRY(db->h_io.grow(cap, kfail, "pinned query I/O block"));
    return ORBX_OK;
}

// Make room for one more slot of n entries: drop erased slots and, if still short, move to larger buffers.  The slot order
// (the add order) is kept.  The compaction reads the old arena, so this is the one growth that keeps its content: the new buffers
// are allocated first and moved in on success; on any failure they go with this scope and the database is as it was.
int orbk_make_room(orbk_database *db, int n)
{
    if ((int)db->slots.size() < db->cap_slots() && db->tail + n <= db->cap_entries()) return ORBX_OK;
    const long long new_ce = std::max(db->cap_entries(), 2 * (db->live_entries + n));
    const int new_cs = std::max(db->cap_slots(), 2 * (db->nlive + 1));
    KHIP(hipStreamSynchronize(db->stream));
    DevBuf<int32_t> n_ids; DevBuf<double> n_vals; DevBuf<KSlotDev> n_slots; DevBuf<long long> d_plan;
    KTRY(n_ids.grow((size_t)new_ce * 4, kfail, "keyframe arena word ids"));
    KTRY(n_vals.grow((size_t)new_ce * 8, kfail, "keyframe arena values"));
    KTRY(n_slots.grow((size_t)new_cs * sizeof(KSlotDev), kfail, "keyframe slot table"));
    std::vector<long long> plan;
    std::vector<KSlotDev> table;
    std::vector<KSlot> kept;
    long long off = 0;
    for (const KSlot &s : db->slots) {
        if (!s.live) continue;
        if (s.len > 0) { plan.push_back(s.off); plan.push_back(off); plan.push_back(s.len); }
        KSlot t = s; t.off = off;
        table.push_back(KSlotDev{off, s.len, 0});
        kept.push_back(t);
        off += s.len;
    }
    const int nplan = (int)(plan.size() / 3);
    if (nplan > 0) {
        KTRY(d_plan.grow(plan.size() * 8, kfail, "keyframe compaction plan"));
        KHIP(hipMemcpy(d_plan, plan.data(), plan.size() * 8, hipMemcpyHostToDevice));
        KHIP(orbk_launch_compact(db->d_ids, db->d_vals, n_ids, n_vals, d_plan, nplan, db->stream));
    }
    if (!table.empty()) KHIP(hipMemcpyAsync(n_slots, table.data(), table.size() * sizeof(KSlotDev), hipMemcpyHostToDevice, db->stream));
    KHIP(hipStreamSynchronize(db->stream));
    db->d_ids = std::move(n_ids); db->d_vals = std::move(n_vals); db->d_slots = std::move(n_slots);
    db->slots.swap(kept);
    db->tail = off;
    db->slot_of.clear();
    for (int i = 0; i < (int)db->slots.size(); i++) db->slot_of[db->slots[i].id] = i;
    return ORBX_OK;
}

extern "C" void orbk_destroy(orbk_database *db)
{
    if (!db) return;
    (void)hipSetDevice(db->device);
    if (db->stream) { (void)hipStreamSynchronize(db->stream); (void)hipStreamDestroy(db->stream); }
    delete db;
}

extern "C" int orbk_create(orbk_database **out, int device, int nwords, int scoring, int max_keyframes, int max_entries)
{
    if (!out) return kfail(ORBX_E_INVALID, "NULL argument");
    *out = nullptr;
    if (nwords <= 0) return kfail(ORBX_E_INVALID, "nwords = %d", nwords);
    if (scoring != ORBV_L1_NORM) return kfail(ORBX_E_INVALID, "scoring type %d: the keyframe database scores with L1 only", scoring);
    if (max_keyframes < 0 || max_entries < 0) return kfail(ORBX_E_INVALID, "negative capacity");
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return kfail(ORBX_E_HIP, "no HIP device: liborbx has no CPU path (%s)", hipGetErrorString(e));
    if (device < 0 || device >= ndev) return kfail(ORBX_E_INVALID, "device %d of %d", device, ndev);
    KHIP(hipSetDevice(device));
    orbk_database *db = new orbk_database();
    db->device = device; db->nwords = nwords;
    const size_t cap_slots = (size_t)std::max(max_keyframes, 4), cap_entries = (size_t)std::max(max_entries, 256);
    if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess ||
        db->d_ids.grow(cap_entries * 4, kfail, "keyframe arena word ids") != ORBX_OK ||
        db->d_vals.grow(cap_entries * 8, kfail, "keyframe arena values") != ORBX_OK ||
        db->d_slots.grow(cap_slots * sizeof(KSlotDev), kfail, "keyframe slot table") != ORBX_OK) {
        orbk_destroy(db);
        return kfail(ORBX_E_HIP, "keyframe database allocation failed");
    }
    *out = db;
    return ORBX_OK;
}
