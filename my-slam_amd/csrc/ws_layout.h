// ws_layout.h -- host-only.  One typed carve of a workspace block: take() a part for each pointer field (its element size times its
// count, rounded up to 64 bytes, in the order taken), ask bytes() for the block's size, then bind() the base and every field points
// at its part.  A part of count 0 gets the address of whatever follows.  The fields stay where they are between take() and bind().
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

class WsLayout {
    void *field_[32];                                   // 32 parts at the most: the largest carve, LBA / BA's, has 27
    size_t off_[32], bytes_ = 0;
    int n_ = 0;
public:
    template <class T> void take(T *&field, size_t count)
    {
        if (n_ >= 32) abort();                          // one part more is a change of the code: raise the bound with it
        field_[n_] = &field; off_[n_++] = bytes_;
        bytes_ += (sizeof(T) * count + 63) & ~(size_t)63;
    }
    size_t bytes() const { return bytes_; }
    void bind(void *base) const
    {
        for (int i = 0; i < n_; i++) {
            uint8_t *at = static_cast<uint8_t *>(base) + off_[i];
            memcpy(field_[i], &at, sizeof at);          // the field is a T * of some T: all object pointers have this representation
        }
    }
};
