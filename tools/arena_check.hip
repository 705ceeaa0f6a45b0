// Host-side check of the measuring pass of the workspace arena (csrc/common.h: Arena; csrc/solver_common.h: arena_open).  Plain C++
// on the CPU: Arena::reserve is replaced by malloc here, nothing is launched and no device is needed.  Build for the host with the
// sanitizers and run:
//
//     hipcc --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined tools/arena_check.hip -o arena_check
//     ./arena_check
//
// It prints one line per check and exits with the number of failed ones.
#include "../jstsp19_amd/csrc/solver_common.h"
#include <cstdlib>
#include <cstring>

namespace jstsp {
static char g_msg[512];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
}
int Arena::reserve(size_t bytes)          // exactly `bytes`: an array more than was measured does not fit
{
    if (bytes <= cap) return 0;
    free(base);
    base = static_cast<char *>(malloc(bytes));
    cap = base ? bytes : 0;
    return base ? 0 : JSTSP_E_NOMEM;
}
void Arena::release() { free(base); base = nullptr; cap = off = 0; }
}  // namespace jstsp

using namespace jstsp;

static int failed = 0;
static void expect(bool ok, const char *what)
{
    printf("%s  %s\n", ok ? "ok  " : "FAIL", what);
    failed += !ok;
}

int main()
{
    // ---- a measuring arena: no memory, the offsets of a real one, the high-water mark across a rewind
    for (int cond = 0; cond < 2; ++cond) {
        Arena m = Arena::measuring();
        float *x = m.get<float>(100);                       // 400 -> 512 bytes
        if (cond) (void)m.get<double>(1);                   // 256
        const size_t mark = m.off;
        (void)m.get<char>(5000);                            // 5120, given back
        m.off = mark;
        (void)m.get<char>(300);                             // 512, over the start of what was given back
        const size_t head = 512 + (cond ? 256 : 0);
        expect(!x && !m.base && m.off == head + 512 && m.peak == head + 5120 && !m.overrun,
               cond ? "measuring arena, conditional array taken: end and peak" : "measuring arena, conditional array absent: end and peak");
    }

    jstsp_ctx ctx;
    // ---- arena_open: the layout of the call is the one that was measured
    {
        float *a1 = nullptr;
        double *a2 = nullptr;
        char *tmp = nullptr, *a3 = nullptr;
        const float caller[4] = {1.f, 2.f, 3.f, 4.f};
        const float *in = nullptr;
        const bool cond = true;
        const int rc = arena_open(&ctx, "consistent", [&](Arena &a) {
            in = a.in(caller, 4, JSTSP_DEVICE);             // (the device path: the caller's pointer, nothing taken)
            a1 = a.get<float>(100);
            a2 = cond ? a.get<double>(33) : nullptr;
            const size_t mark = a.off;
            tmp = a.get<char>(5000);
            a.off = mark;
            a3 = a.get<char>(300);
        });
        Arena &a = ctx.arena;
        expect(rc == 0 && in == caller, "arena_open: a consistent layout opens");
        expect(a.cap == 512 + 512 + 5120 && a.peak == a.cap && a.off == 512 + 512 + 512, "arena_open: the arena holds the measured peak");
        expect((char *)a1 == a.base && (char *)a2 == a.base + 512 && tmp == a.base + 1024 && a3 == tmp, "arena_open: offsets in the order of the calls");
        memset(a.base, 0x5a, a.cap);                        // every byte of the peak is ours (the sanitizer watches)
    }
    // ---- a layout whose second pass takes one array more is refused, and nothing after arena_open runs
    {
        ctx.arena.release();
        int pass = 0;
        bool ran = false;
        const auto call = [&]() -> int {
            JSTSP_TRY(arena_open(&ctx, "inconsistent", [&](Arena &a) {
                (void)a.get<float>(100);
                if (pass++ > 0) (void)a.get<float>(1);
            }));
            ran = true;
            return 0;
        };
        const int rc = call();
        expect(rc == JSTSP_E_NOMEM && !ran && pass == 2, "arena_open: an inconsistent layout is refused, not run");
        expect(strstr(g_msg, "inconsistent: internal error") != nullptr && ctx.arena.overrun, "arena_open: the refusal names the entry");
        printf("      message: %s\n", g_msg);
        // (the same with room to spare - a grown arena of an earlier call: the ends differ)
        JSTSP_TRY(ctx.arena.reserve(1 << 16));
        pass = 0;
        expect(call() == JSTSP_E_NOMEM && !ran && !ctx.arena.overrun, "arena_open: ... also when the extra array fits the arena");
        printf("      message: %s\n", g_msg);
    }
    // ---- a real arena past its end: nullptr, the flag stays until reset()
    {
        Arena &a = ctx.arena;
        a.reset();
        char *big = a.get<char>(a.cap + 1), *small = a.get<char>(1);
        expect(!big && small == a.base && a.overrun, "real arena: a get past the end sets the flag and later ones go on");
        a.reset();
        expect(!a.overrun && a.off == 0 && a.peak == 0, "real arena: reset() clears it");
    }
    ctx.arena.release();
    printf("%d check(s) failed\n", failed);
    return failed;
}
