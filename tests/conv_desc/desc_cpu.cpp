// The launch rules of loans_amd/csrc/conv_desc.h as a plain C++ program (see test_desc_cpu.py): reads cases on stdin, prints
// one line per case with one character per check -- K = LOANS_OK, I = LOANS_EINVAL, R = LOANS_ERANGE, 1 / 0 = covered / not,
// '-' = not asked (the geometry predicates read a tap list of 1 .. LOANS_MAX_TAPS entries).
// A case: n focus splits Cout_b have misaligned w_have, then n descriptors of 18 fields + 64 dy + 64 dx.
// `mark` as first argument: every check runs in a child process of its own, and '!' stands where UBSan (the build is
// -fsanitize=undefined -fno-sanitize-recover) stopped the child on a signed integer overflow.
#include <stdio.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>
#include "conv_desc.h"

static const unsigned HAVE_W_LIST = 1u << 13;       // the array of class weight pointers (no CONV_P_* bit: only the class entry has it)

static char code(int rc) { return rc == LOANS_OK ? 'K' : rc == LOANS_EINVAL ? 'I' : rc == LOANS_ERANGE ? 'R' : '?'; }

#ifdef CONV_DESC_MOVED       // built against the move-only commit's header, whose checks handed no byte sizes back
#define BYTES
#else
#define BYTES , &bytes
#endif

// f() in a child process: its answer, or '!' when UBSan stopped it on a signed integer overflow, '?' when it died of anything else
template <typename F>
static char in_child(F f) {
    fflush(stdout);
    int fd[2];
    if (pipe(fd)) return '?';
    const pid_t pid = fork();
    if (pid == 0) {
        dup2(fd[1], 2);
        _exit(f());
    }
    close(fd[1]);
    char text[4096];
    size_t n = 0;
    for (ssize_t r; n + 1 < sizeof text && (r = read(fd[0], text + n, sizeof text - 1 - n)) > 0;) n += (size_t)r;
    text[n] = 0;
    close(fd[0]);
    int st = 0;
    if (pid < 0 || waitpid(pid, &st, 0) != pid) return '?';
    if (WIFEXITED(st) && WEXITSTATUS(st) >= '-') return (char)WEXITSTATUS(st);
    return strstr(text, "signed integer overflow") ? '!' : '?';
}

static bool read_desc(loans_igemm_desc* d) {
    int32_t* f = &d->B;
    for (int i = 0; i < 18; ++i)
        if (scanf("%d", f + i) != 1) return false;
    for (int k = 0; k < 2; ++k)
        for (int i = 0; i < LOANS_MAX_TAPS; ++i) {
            int v;
            if (scanf("%d", &v) != 1) return false;
            (k ? d->dx : d->dy)[i] = (int8_t)v;
        }
    return true;
}

int main(int argc, char** argv) {
    const bool mark = argc > 1 && !strcmp(argv[1], "mark");
    static_assert(sizeof(loans_igemm_desc) == 18 * 4 + 2 * LOANS_MAX_TAPS, "the descriptor is read field by field");
    int n, focus, splits, cout_b;
    unsigned have, mis, w_have;
    while (scanf("%d %d %d %d %u %u %u", &n, &focus, &splits, &cout_b, &have, &mis, &w_have) == 7) {
        loans_igemm_desc descs[LOANS_MAX_CLASSES];
        if (n < 1 || n > LOANS_MAX_CLASSES || focus < 0 || focus >= n) return 2;
        for (int c = 0; c < n; ++c)
            if (!read_desc(descs + c)) return 2;
        const loans_igemm_desc* d = descs + focus;
        const int64_t rows = (int64_t)d->B * d->gridH * d->gridW;
        const bool taps_ok = d->ntaps >= 1 && d->ntaps <= LOANS_MAX_TAPS;
        loans_igemm_desc stacked;
#ifndef CONV_DESC_MOVED
        ConvBytes bytes;
#endif
        int64_t nblk;
        char out[32];
        int k = 0;
#define CHECK(expr) do { out[k] = mark ? in_child([&] { return (char)(expr); }) : (char)(expr); ++k; } while (0)
        CHECK(code(conv_check_igemm32(d, have, mis, 0)));
        CHECK(code(conv_check_igemm32(d, have, mis, 1)));
        CHECK(code(conv_check_igemm_pair_f32(d, have, mis, cout_b)));
        CHECK(code(conv_check_igemm_classes_f32(descs, n, have, mis, have & HAVE_W_LIST, w_have)));
        CHECK(code(conv_check_igemm16(d, have & ~(CONV_P_PARTIAL | HAVE_W_LIST), mis)));
        CHECK(code(conv_check_igemm_pair_bf16s(d, have, mis, &stacked)));
        CHECK(code(conv_check_igemm16(d, have & (CONV_P_IN | CONV_P_W | CONV_P_PARTIAL), mis, splits)));
        CHECK(code(conv_check_finalize_f32(have, d->flags, rows, d->Cout)));
        CHECK(code(conv_check_finalize_bf16(have, d->flags, rows, d->Cout, &nblk)));
        CHECK(code(conv_check_wgrad32(d, have, mis, 0 BYTES)));
        CHECK(code(conv_check_wgrad32(d, have, mis, 1 BYTES)));
        CHECK(code(conv_check_wgrad_bf16s(d, have, mis, false, false, false BYTES)));
        CHECK(code(conv_check_wgrad_bf16s(d, have, mis, false, true, false BYTES)));
        CHECK(code(conv_check_wgrad_bf16s(d, have, mis, false, true, true BYTES)));
        CHECK(code(conv_check_wgrad_bf16s(d, 0, 0, true, false, false BYTES)));
        CHECK(taps_ok ? '0' + conv_halo16_covers(d, d->tile) : '-');
        CHECK(taps_ok ? '0' + conv_pw16_covers(d) : '-');
        CHECK(taps_ok ? '0' + conv_stem7_wgrad_bf16_covers(d) : '-');
#undef CHECK
        out[k] = 0;
        puts(out);
    }
    return 0;
}
