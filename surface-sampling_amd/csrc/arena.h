// arena.h -- the one carver of the drivers' workspaces: a buffer that holds several typed blocks is described once, as a function
// that calls place(field, count) per block in buffer order, and that function is run twice -- by a sizing Arena, which only adds
// up, and by an Arena at the buffer's base, which hands out the pointers.  Size and pointers cannot drift apart: there is no
// second formula.  Plain C++17, no HIP, nothing of the handle: a host program can include this header alone (tests/arena_layout.cpp).
#ifndef VSSR_ARENA_H
#define VSSR_ARENA_H
#include <algorithm>
#include <cstddef>

namespace vssr {

class Arena {
    char *base_;
    bool sizing_;
    size_t block_align_, off_ = 0;
    Arena(char *base, bool sizing, size_t block_align) : base_(base), sizing_(sizing), block_align_(block_align) {}

public:
    // block_align 1: every block at the natural alignment of its type; 256: every block on a 256-byte line of its own
    static Arena sizing(size_t block_align = 1) { return Arena(nullptr, true, block_align); }
    static Arena at(void *base, size_t block_align = 1) { return Arena(static_cast<char *>(base), false, block_align); }

    void align(size_t a) { off_ = (off_ + a - 1) / a * a; }
    template <class T>
    void place(T *&field, size_t count) {
        align(std::max(alignof(T), block_align_));
        if (!sizing_) field = reinterpret_cast<T *>(base_ + off_);
        off_ += count * sizeof(T);
    }
    size_t offset() const { return off_; }   // bytes placed so far: the total after the last place, a span's end in between
};

// bytes `layout` needs; the pointers of `layout` in the buffer at `base` (returns the bytes as well)
template <class Layout>
size_t arena_size(Layout &&layout, size_t block_align = 1) {
    Arena a = Arena::sizing(block_align);
    layout(a);
    return a.offset();
}
template <class Layout>
size_t arena_carve(void *base, Layout &&layout, size_t block_align = 1) {
    Arena a = Arena::at(base, block_align);
    layout(a);
    return a.offset();
}

}  // namespace vssr
#endif
