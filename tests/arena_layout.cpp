// The drivers' workspace layouts on the carver of csrc/arena.h, on the host: every layout is carved over a malloc of exactly the size
// the sizing pass measured, every block's offset and the total are compared with the formulas the drivers used before the carver
// (written out here a second time, on purpose: running counts of doubles and ints, as the entry points had them), every pointer
// is tested for its type's alignment, and every element of every block is written -- built with -fsanitize=address,undefined
// (tests/test_arena_cpu.py), which is the judge of "inside the allocation".  Includes arena.h alone; the structs are stand-ins with
// the sizes and alignments of the device structs they name.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "arena.h"

using vssr::Arena;

struct NebChain { int first, idx, nimg, band; };                          // neb_dev.h
struct VibChain { int group, rank, nrep, m; };                            // vib.hip
struct VibState { int j, s, reason, pad; };
struct DimerState { double d[6]; int i[8]; };                             // dimer.hip: 80 bytes, aligned 8
struct CellState { double d[39]; int i[7]; };                             // relax_cell.hip: 340 bytes padded to 344, aligned 8
struct CgState { int i[6]; double d[10]; };                               // cg_dev.h: 104 bytes, aligned 8
static_assert(sizeof(NebChain) == 16 && sizeof(VibChain) == 16 && sizeof(VibState) == 16 && sizeof(DimerState) == 80 &&
              sizeof(CellState) == 344 && sizeof(CgState) == 104, "stand-in sizes");
constexpr size_t NEB_SLOT = 8;

static int failures = 0;
#define CHECK(cond, ...) \
    do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

// One carved block as the test sees it: where it is, how long, how aligned it must be, and the offset the old formula gives
struct Block { const char *name; void *p; size_t bytes, align, want; };
template <class T>
static Block block(const char *name, T *p, size_t count, size_t want) { return {name, p, count * sizeof(T), alignof(T), want}; }

// sizing pass, malloc of exactly that, pointer pass, then the checks.  `blocks` is called after the pointer pass.
template <class Layout, class Blocks>
static void run(const char *what, size_t want_total, size_t block_align, Layout layout, Blocks blocks) {
    const size_t total = vssr::arena_size(layout, block_align);
    CHECK(total == want_total, "%s: total %zu, the old formula gives %zu", what, total, want_total);
    char *base = static_cast<char *>(std::malloc(total));
    const size_t again = vssr::arena_carve(base, layout, block_align);
    CHECK(again == total, "%s: the pointer pass ends at %zu, the sizing pass at %zu", what, again, total);
    unsigned char fill = 1;
    for (const Block &b : blocks()) {
        const size_t off = static_cast<size_t>(static_cast<char *>(b.p) - base);
        CHECK(off == b.want, "%s.%s: offset %zu, the old formula gives %zu", what, b.name, off, b.want);
        CHECK(reinterpret_cast<uintptr_t>(b.p) % b.align == 0, "%s.%s: not aligned to %zu", what, b.name, b.align);
        CHECK(off + b.bytes <= total, "%s.%s: ends at %zu of %zu", what, b.name, off + b.bytes, total);
        std::memset(b.p, fill++, b.bytes);   // every element; past the malloc: AddressSanitizer stops the program
    }
    std::free(base);
}

struct Shape { size_t B, N, g, vib_len, ld, nrec; };   // g: bands / dimers / groups

static void neb(const Shape &s) {
    const size_t n3 = 3 * s.N, B = s.B, nb = s.g, D = sizeof(double), I = sizeof(int);
    double *G, *slot, *band; NebChain *ch; int *binfo, *gfirst, *flags;
    size_t dbl_bytes = 0;
    const size_t n_dbl = n3 + NEB_SLOT * B + 3 * nb, n_int = 4 * B + 5 * nb + 4;
    run("d_neb", D * n_dbl + I * n_int, 1,
        [&](Arena &a) {
            a.place(G, n3); a.place(slot, NEB_SLOT * B); a.place(band, 3 * nb);
            dbl_bytes = a.offset();
            a.place(ch, B); a.place(binfo, 4 * nb); a.place(gfirst, nb); a.place(flags, 4);
        },
        [&] {
            size_t d = 0, ip;
            std::vector<Block> v;
            v.push_back(block("G", G, n3, D * d)); d += n3;
            v.push_back(block("slot", slot, NEB_SLOT * B, D * d)); d += NEB_SLOT * B;
            v.push_back(block("band", band, 3 * nb, D * d)); d += 3 * nb;
            ip = 0;
            v.push_back(block("ch", ch, B, D * d + I * ip)); ip += 4 * B;
            v.push_back(block("binfo", binfo, 4 * nb, D * d + I * ip)); ip += 4 * nb;
            v.push_back(block("gfirst", gfirst, nb, D * d + I * ip)); ip += nb;
            v.push_back(block("flags", flags, 4, D * d + I * ip));
            return v;
        });
    CHECK(dbl_bytes == D * n_dbl, "d_neb: the cleared span is %zu bytes, n_dbl doubles are %zu", dbl_bytes, D * n_dbl);
}

static void dimer(const Shape &s) {
    const size_t n3 = 3 * s.N, B = s.B, ng = s.g, D = sizeof(double), I = sizeof(int);
    double *N, *Nopen, *xopen, *F0, *F1, *theta, *vel, *rec; unsigned long long *ids; DimerState *st; NebChain *ch; int *info, *flags;
    size_t dbl_bytes = 0;
    const size_t n_dbl = 7 * n3 + 4 * ng, n_int = 4 * B + 4 * ng + 4;
    run("d_dimer", D * n_dbl + sizeof(unsigned long long) * ng + sizeof(DimerState) * ng + I * n_int, 1,
        [&](Arena &a) {
            a.place(N, n3); a.place(Nopen, n3); a.place(xopen, n3); a.place(F0, n3); a.place(F1, n3);
            a.place(theta, n3); a.place(vel, n3); a.place(rec, 4 * ng);
            dbl_bytes = a.offset();
            a.place(ids, ng); a.place(st, ng);
            a.place(ch, B); a.place(info, 4 * ng); a.place(flags, 4);
        },
        [&] {
            std::vector<Block> v;
            double *seven[7] = {N, Nopen, xopen, F0, F1, theta, vel};
            const char *names[7] = {"N", "Nopen", "xopen", "F0", "F1", "theta", "vel"};
            for (size_t k = 0; k < 7; ++k) v.push_back(block(names[k], seven[k], n3, D * k * n3));
            v.push_back(block("rec", rec, 4 * ng, D * 7 * n3));
            const size_t o_ids = D * n_dbl, o_st = o_ids + 8 * ng, o_int = o_st + sizeof(DimerState) * ng;
            v.push_back(block("ids", ids, ng, o_ids));
            v.push_back(block("st", st, ng, o_st));
            v.push_back(block("ch", ch, B, o_int));
            v.push_back(block("info", info, 4 * ng, o_int + I * 4 * B));
            v.push_back(block("flags", flags, 4, o_int + I * (4 * B + 4 * ng)));
            return v;
        });
    CHECK(dbl_bytes == D * n_dbl, "d_dimer: the cleared span is %zu bytes, n_dbl doubles are %zu", dbl_bytes, D * n_dbl);
}

static void cellrelax(const Shape &s) {
    const size_t n3 = 3 * s.N, B = s.B, D = sizeof(double), I = sizeof(int);
    double *sc, *sopen, *vel, *rec; CellState *st; int *info, *flags;
    const size_t n_dbl = 3 * n3 + 3 * B;
    run("d_cellrelax", D * n_dbl + sizeof(CellState) * B + I * (2 * B + 2), 1,
        [&](Arena &a) {
            a.place(sc, n3); a.place(sopen, n3); a.place(vel, n3); a.place(rec, 3 * B);
            a.place(st, B); a.place(info, 2 * B); a.place(flags, 2);
        },
        [&] {
            const size_t o_st = D * n_dbl, o_int = o_st + sizeof(CellState) * B;
            return std::vector<Block>{block("s", sc, n3, 0), block("sopen", sopen, n3, D * n3), block("vel", vel, n3, D * 2 * n3),
                                      block("rec", rec, 3 * B, D * 3 * n3), block("st", st, B, o_st), block("info", info, 2 * B, o_int),
                                      block("flags", flags, 2, o_int + I * 2 * B)};
        });
}

static void vib(const Shape &s) {
    const size_t N = s.N, n3 = 3 * N, B = s.B, G = s.g, ldd = s.ld, mat = G * ldd * ldd, len = s.vib_len, D = sizeof(double), I = sizeof(int);
    double *x0, *Fs, *mass, *K, *Hs, *A, *W, *Vt, *w2, *en, *thermo; VibChain *ch; VibState *st;
    int *vib_start, *vib_list, *gm, *gfirst, *gbad, *jinfo, *info, *flags;
    const size_t n_dbl = n3 * 5 + N + 5 * mat + 2 * G * ldd + 3 * G;
    const size_t n_int = 4 * B * 2 + (B + 1) + len + 1 + 9 * G + 4;
    run("d_vib", D * n_dbl + I * n_int, 1,
        [&](Arena &a) {
            a.place(x0, n3); a.place(Fs, 4 * n3); a.place(mass, N);
            a.place(K, mat); a.place(Hs, mat); a.place(A, mat); a.place(W, mat); a.place(Vt, mat);
            a.place(w2, G * ldd); a.place(en, G * ldd); a.place(thermo, 3 * G);
            a.place(ch, B); a.place(st, B);
            a.place(vib_start, B + 1); a.place(vib_list, len + 1);
            a.place(gm, G); a.place(gfirst, G); a.place(gbad, G); a.place(jinfo, 2 * G); a.place(info, 4 * G);
            a.place(flags, 4);
        },
        [&] {
            std::vector<Block> v;
            size_t d = 0;
            v.push_back(block("x0", x0, n3, D * d)); d += n3;
            v.push_back(block("Fs", Fs, 4 * n3, D * d)); d += 4 * n3;
            v.push_back(block("mass", mass, N, D * d)); d += N;
            v.push_back(block("K", K, mat, D * d)); d += mat;
            v.push_back(block("Hs", Hs, mat, D * d)); d += mat;
            v.push_back(block("A", A, mat, D * d)); d += mat;
            v.push_back(block("W", W, mat, D * d)); d += mat;
            v.push_back(block("Vt", Vt, mat, D * d)); d += mat;
            v.push_back(block("w2", w2, G * ldd, D * d)); d += G * ldd;
            v.push_back(block("en", en, G * ldd, D * d)); d += G * ldd;
            v.push_back(block("thermo", thermo, 3 * G, D * d)); d += 3 * G;
            size_t ip = 0;
            v.push_back(block("ch", ch, B, D * d + I * ip)); ip += 4 * B;
            v.push_back(block("st", st, B, D * d + I * ip)); ip += 4 * B;
            v.push_back(block("vib_start", vib_start, B + 1, D * d + I * ip)); ip += B + 1;
            v.push_back(block("vib_list", vib_list, len + 1, D * d + I * ip)); ip += len + 1;
            v.push_back(block("gm", gm, G, D * d + I * ip)); ip += G;
            v.push_back(block("gfirst", gfirst, G, D * d + I * ip)); ip += G;
            v.push_back(block("gbad", gbad, G, D * d + I * ip)); ip += G;
            v.push_back(block("jinfo", jinfo, 2 * G, D * d + I * ip)); ip += 2 * G;
            v.push_back(block("info", info, 4 * G, D * d + I * ip)); ip += 4 * G;
            v.push_back(block("flags", flags, 4, D * d + I * ip));
            return v;
        });
}

static void md_aux(const Shape &s, size_t nrec) {
    const size_t B = s.B;
    int *stopped; unsigned long long *ids; double *thermo;
    const size_t aux_ids = 16, aux_thermo = 16 + sizeof(unsigned long long) * B;   // the old aux_ids() / aux_thermo(B)
    run(nrec ? "d_md_aux" : "d_md_aux (ids only)", aux_thermo + sizeof(double) * 2 * B * nrec, 1,
        [&](Arena &a) { a.place(stopped, 4); a.place(ids, B); a.place(thermo, 2 * B * nrec); },
        [&] {
            return std::vector<Block>{block("stopped", stopped, 4, 0), block("ids", ids, B, aux_ids),
                                      block("thermo", thermo, 2 * B * nrec, aux_thermo)};
        });
}

static void cm(const Shape &s) {
    const size_t B = s.B;
    char *args; int *flags, *n_evals;
    run("d_cm", sizeof(int) * (B + 8) + 1024, 1, [&](Arena &a) { a.place(args, 1024); a.place(flags, 8); a.place(n_evals, B); },
        [&] {
            return std::vector<Block>{block("args", args, 1024, 0), block("flags", flags, 8, 1024),
                                      block("n_evals", n_evals, B, 1024 + sizeof(int) * 8)};
        });
}

// The compaction arena: [orig (inputs and results) | maps | tmp (every field)], every block rounded up to 256 bytes
struct CmpView {
    int *cfg_start, *Z, *atom_cfg, *nimg;
    double *pos, *cell, *inv, *x0, *hh, *gg;
    uint8_t *pbc, *fixed;
    CgState *st;
};
static void cmp(const Shape &s) {
    const size_t B = s.B, N = s.N;
    CmpView orig{}, tmp{};
    int *live = nullptr, *live_new = nullptr, *src = nullptr, *start_new = nullptr, *totals = nullptr;
    auto fields = [&](Arena &a, CmpView &v, bool work) {   // the order of for_each_field (relax_cg.hip)
        a.place(v.cfg_start, B + 1); a.place(v.Z, N); a.place(v.atom_cfg, N); a.place(v.nimg, 3 * B); a.place(v.pos, 3 * N);
        a.place(v.cell, 9 * B); a.place(v.inv, 9 * B);
        if (work) { a.place(v.x0, 3 * N); a.place(v.hh, 3 * N); a.place(v.gg, 3 * N); }
        a.place(v.pbc, 3 * B); a.place(v.fixed, N); a.place(v.st, B);
    };
    std::vector<Block> want;
    size_t off = 0;
    auto old_place = [&](const char *name, auto *p, size_t n) {   // the old carve: off += (n * sizeof + 255) & ~255
        want.push_back(block(name, p, n, off));
        off += (n * sizeof(*p) + 255) & ~(size_t)255;
    };
    auto old_fields = [&](CmpView &v, bool work) {
        old_place("cfg_start", v.cfg_start, B + 1); old_place("Z", v.Z, N); old_place("atom_cfg", v.atom_cfg, N);
        old_place("nimg", v.nimg, 3 * B); old_place("pos", v.pos, 3 * N); old_place("cell", v.cell, 9 * B); old_place("inv", v.inv, 9 * B);
        if (work) { old_place("x0", v.x0, 3 * N); old_place("hh", v.hh, 3 * N); old_place("gg", v.gg, 3 * N); }
        old_place("pbc", v.pbc, 3 * B); old_place("fixed", v.fixed, N); old_place("st", v.st, B);
    };
    auto old_all = [&] {
        want.clear(); off = 0;
        old_fields(orig, false);
        old_place("live", live, B); old_place("live_new", live_new, B); old_place("src", src, B); old_place("start_new", start_new, B + 1);
        old_place("totals", totals, (size_t)4);
        old_fields(tmp, true);
    };
    old_all();   // (for the total: the pointers are not set yet, only the offsets count)
    run("d_cmp", off, 256,
        [&](Arena &a) {
            fields(a, orig, false);
            a.place(live, B); a.place(live_new, B); a.place(src, B); a.place(start_new, B + 1); a.place(totals, 4);
            fields(a, tmp, true);
            a.align(256);
        },
        [&] { old_all(); return want; });
}

int main() {
    // per driver the degenerate shape, then one ragged shape with odd counts: int blocks end off an 8-byte boundary
    const Shape one{1, 1, 1, 0, 1, 1}, ragged{5, 7, 3, 5, 3, 3};
    neb(Shape{3, 1, 1, 0, 1, 1});
    dimer(Shape{2, 1, 1, 0, 1, 1});
    cellrelax(one); vib(one); md_aux(one, one.nrec); md_aux(one, 0); cm(one); cmp(one);
    neb(ragged); dimer(ragged); cellrelax(ragged); vib(ragged); md_aux(ragged, ragged.nrec); md_aux(ragged, 0);
    cm(ragged); cmp(ragged);
    std::printf("%s: %d failure(s)\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
