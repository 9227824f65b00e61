// Device staging of ONE call of a host-pointer entry (bmpc_fk, bmpc_ik, bmpc_convex_sets): the caller names its arrays, run() makes
// the one allocation, uploads, launches, downloads, waits and frees.  (bmpc_solve keeps persistent buffers on the handle instead:
// it is called in a loop, these entries are not.)
//     Staging s;
//     s.in(&x, n);  s.out(&y, m);            // x, y: the entry's own host-pointer arguments
//     return s.run(h, st, [&]() -> int { HIPCHK(h, launch(x, y, st)); return 0; });
// in() / out() take the ADDRESS of a pointer variable that holds the host array; run() points that variable at the device copy
// before it uploads, so the launch is written once, on the same names, whether they hold the caller's device pointers (the _dev
// entries, which do not stage) or staged host arrays.  An optional array the caller left out (pointer null) takes no room and
// stays null, which is how the kernels are told to skip it.
#pragma once
#include "bmpc_handle.hpp"

#include <cstring>
#include <functional>
#include <vector>

class __attribute__((visibility("hidden"))) Staging {       // (not part of the exported symbol set)
public:
    template <class T> void in(T** p, size_t count) { add(p, host_of(*p), count * sizeof(T), IN); }
    template <class T> void out(T** p, size_t count) { add(p, host_of(*p), count * sizeof(T), OUT); }
    template <class T> void scratch(T** p, size_t count) { add(p, nullptr, count * sizeof(T), SCRATCH); }   // device only, *p ignored

    // Everything on `st`, in order: uploads, what `launch` enqueues (it returns an entry point's code, 0 = go on), downloads, then
    // the wait.  The registered pointers are device pointers from here on, valid inside `launch` only.
    int run(bmpc_handle* h, hipStream_t st, const std::function<int()>& launch) {
        void* blk = nullptr;
        const int rc = enqueue(h, st, launch, &blk);
        // freed on the error paths too -- except after the watchdog fired: work still queued on the stream may write the block,
        // and hipFree would wait for a stream that may never drain; it is leaked, as bmpc_destroy leaks the workspace
        if (blk && !h->wedged) (void)hipFree(blk);
        return rc;
    }

private:
    enum Dir { IN, OUT, SCRATCH };
    struct Item { void* var; void* host; size_t off, bytes; Dir dir; };      // var: address of the caller's pointer variable
    static constexpr size_t ALIGN = 256;      // of every array inside the block (hipMalloc aligns the block itself to at least that)
    std::vector<Item> items_;
    size_t total_ = 0;

    static void* host_of(const void* p) { return const_cast<void*>(p); }
    void add(void* var, void* host, size_t bytes, Dir dir) {
        if (bytes == 0 || (dir != SCRATCH && !host)) return;
        items_.push_back({var, host, total_, bytes, dir});
        total_ += (bytes + ALIGN - 1) / ALIGN * ALIGN;
    }
    int enqueue(bmpc_handle* h, hipStream_t st, const std::function<int()>& launch, void** blk) {
        HIPCHK(h, hipMalloc(blk, total_));
        for (const Item& it : items_) {
            void* p = (char*)*blk + it.off;
            std::memcpy(it.var, &p, sizeof p);      // (a T* through its address: every object pointer has this representation)
            if (it.dir == IN) HIPCHK(h, hipMemcpyAsync(p, it.host, it.bytes, hipMemcpyHostToDevice, st));
        }
        if (int r = launch()) return r;
        for (const Item& it : items_)
            if (it.dir == OUT) HIPCHK(h, hipMemcpyAsync(it.host, (char*)*blk + it.off, it.bytes, hipMemcpyDeviceToHost, st));
        return wait_stream(h, st);
    }
};
