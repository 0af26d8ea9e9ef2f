// Stand-alone driver of localization_amd/csrc/window_layouts.h for tests/test_kernel_layouts_cpu.py: host code only, built with plain g++
// under AddressSanitizer + UBSan.  No HIP call, nothing else of the product.
//
//   kernel_layouts_driver <in> <out>
//
// <in>: int64 rows, 6, then rows x {nv_max, bw_max, nr_max, np_max, ns_max, nb_max}.
// <out>: int64 [rows][kWidth], the columns tests/test_kernel_layouts_cpu.py names: every array's offset in BYTES from its block's start
// (-1: the variant has no such array), every total, the predicates and the fit rules.
//
// Besides, for every layout of every row (a failure is a line on stderr and exit status 1):
//   * every array lies inside the total, starts on a multiple of its element size (RecA: 16 bytes), and the int region starts where the
//     doubles end;
//   * a buffer of exactly the total is allocated, every element of every array is written through its carved pointer with the array's own
//     tag, and then read back: an extent that overruns is an AddressSanitizer report, an overlap is a wrong tag.  (Blocks of more than
//     kMaxBuffer bytes — the HBM slices of the longest windows — are checked by interval arithmetic alone.)
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "window_layouts.h"

using namespace locamd;

namespace {

constexpr size_t kMaxBuffer = 48u << 20;
int g_failures = 0;
std::vector<int64_t> g_out;
long long g_row = -1;

void fail(const std::string& block, const std::string& what) {
    if (++g_failures <= 20) std::fprintf(stderr, "row %lld, %s: %s\n", g_row, block.c_str(), what.c_str());
}
void put(int64_t v) { g_out.push_back(v); }

enum { kSilent = 0, kValue = 1, kOptional = 2 };
struct Piece { const char* name; size_t at, len, elem; };   // bytes
struct Block {
    std::string name;
    size_t bytes = 0;
    std::vector<Piece> pieces;
    // an array of `elem`-byte elements, `sp` counted in elements from `base` bytes.  mode kValue: its offset is a column (an empty array's
    // too: the kernel forms that pointer all the same), less `rel`; kOptional: -1 when the variant has no such array; kSilent: no column
    void add(const char* nm, size_t base, Span sp, size_t elem, int mode = 1, size_t rel = 0) {
        if (mode != kSilent) put(sp.n || mode == kValue ? (int64_t)(base + sp.at * elem) - (int64_t)rel : -1);
        if (sp.n) pieces.push_back({nm, base + sp.at * elem, sp.n * elem, elem});
    }
};

template <class T>
void fill(unsigned char* buf, const Piece& p, uint32_t tag) {
    T* q = reinterpret_cast<T*>(buf + p.at);   // (a misaligned array is a UBSan report at the first store)
    for (size_t i = 0; i < p.len / sizeof(T); ++i) q[i] = (T)tag;
}
template <class T>
bool holds(const unsigned char* buf, const Piece& p, uint32_t tag) {
    const T* q = reinterpret_cast<const T*>(buf + p.at);
    for (size_t i = 0; i < p.len / sizeof(T); ++i) if (q[i] != (T)tag) return false;
    return true;
}

void check(const Block& b) {
    std::vector<Piece> s = b.pieces;
    for (const Piece& p : s) {
        if (p.at % p.elem) fail(b.name, std::string(p.name) + " is not aligned to its element");
        if (p.at + p.len > b.bytes) fail(b.name, std::string(p.name) + " ends behind the total");
    }
    std::sort(s.begin(), s.end(), [](const Piece& x, const Piece& y) { return x.at < y.at; });
    for (size_t i = 1; i < s.size(); ++i) if (s[i - 1].at + s[i - 1].len > s[i].at) fail(b.name, std::string(s[i - 1].name) + " overlaps " + s[i].name);
    if (g_failures || b.bytes == 0 || b.bytes > kMaxBuffer) return;
    unsigned char* buf = new unsigned char[b.bytes];
    uint32_t tag = 1;
    for (const Piece& p : b.pieces) {
        if (p.elem == 4) fill<uint32_t>(buf, p, tag); else fill<uint64_t>(buf, p, tag);   // (16-byte records: two words each)
        ++tag;
    }
    tag = 1;
    for (const Piece& p : b.pieces) {
        if (!(p.elem == 4 ? holds<uint32_t>(buf, p, tag) : holds<uint64_t>(buf, p, tag))) fail(b.name, std::string(p.name) + " was overwritten by another array");
        ++tag;
    }
    delete[] buf;
}
void ints_follow(const Block& b, size_t ints_bytes, size_t n_double_arrays) {
    size_t end = 0;
    for (size_t i = 0; i < n_double_arrays && i < b.pieces.size(); ++i) if (b.pieces[i].elem == 8) end = std::max(end, b.pieces[i].at + b.pieces[i].len);
    if (ints_bytes != end) fail(b.name, "the int region does not start where the doubles end");
}

void wave3(const WindowCaps& c, bool pinfo) {
    const W3Layout l = w3_layout(c, pinfo);
    Block b; b.name = pinfo ? "wave3 pinfo" : "wave3"; b.bytes = l.bytes;
    b.add("T", 0, l.T, 8); b.add("rec", 0, l.rec, 8); b.add("ev", 0, l.ev, 8); b.add("fix", 0, l.fix, 8); b.add("pv", 0, l.pv, 8);
    const size_t ib = l.ints * 8;
    b.add("eidx", ib, l.eidx, 4); b.add("epos", ib, l.epos, 4); b.add("pidx", ib, l.pidx, 4);
    put((int64_t)l.bytes);
    ints_follow(b, ib, 5);
    check(b);
}
void wave6(const WindowCaps& c, bool se3) {
    const W6Layout l = w6_layout(c, se3);
    Block b; b.name = se3 ? "wave6 se3" : "wave6"; b.bytes = l.bytes;
    b.add("pose", 0, l.pose, 8); b.add("rec", 0, l.rec, 8); b.add("prec", 0, l.prec, 8); b.add("ev", 0, l.ev, 8); b.add("fix", 0, l.fix, 8); b.add("pv", 0, l.pv, 8);
    b.add("sv", 0, l.sv, 8, kOptional);
    const size_t ib = l.ints * 8;
    b.add("eidx", ib, l.eidx, 4); b.add("epos", ib, l.epos, 4); b.add("pidx", ib, l.pidx, 4); b.add("ppos", ib, l.ppos, 4);
    put((int64_t)l.bytes);
    ints_follow(b, ib, 7);
    check(b);
}
void arrow3(const WindowCaps& c, int nb) {
    const Arrow3Lds l = arrow3_lds_layout(c.nv_max, nb);
    Block b; b.name = "arrow3 lds"; b.bytes = l.bytes;
    b.add("PK", 0, l.PK, 8); b.add("GZ", 0, l.GZ, 8); b.add("C0", 0, l.C0, 8); b.add("S", 0, l.S, 8); b.add("bB", 0, l.bB, 8); b.add("xB", 0, l.xB, 8);
    b.add("xsB", 0, l.xsB, 8); b.add("RA", 0, l.RA, 8); b.add("FX", 0, l.FX, 8); b.add("TB", 0, l.TB, 8); b.add("red", 0, l.red, 8); b.add("AN", 0, l.AN, 8);
    put((int64_t)l.bytes);
    check(b);
    const Arrow3Ws w = arrow3_ws_layout(c, nb);
    Block h; h.name = "arrow3 workspace"; h.bytes = w.doubles * 8;
    h.add("TT", 0, w.TT, 8); h.add("XS", 0, w.XS, 8); h.add("BB", 0, w.BB, 8); h.add("CS", 0, w.CS, 8);
    put((int64_t)h.bytes);
    check(h);
}

void window(const WindowCaps& c, bool ga) {
    const bool sp = window_sparse_path(c);
    const int W = window_mask_words(c);
    const WindowLayout y = window_layout(c, ga);
    const WindowTables& T = y.T;
    const WindowIndex& I = y.I;
    // two blocks in workspace mode (the instance's HBM slice; the LDS), one in LDS mode
    Block m; m.name = ga ? "window workspace" : "window lds"; m.bytes = ga ? y.main_doubles * 8 : y.lds_bytes;
    Block s; s.name = "window lds (workspace mode)"; s.bytes = y.lds_bytes;
    Block& lds = ga ? s : m;
    for (const Span* a : {&y.Hs, &y.Ls, &y.diagL, &y.b, &y.x, &y.yrow, &y.pose, &y.bak, &y.rrec, &y.prec, &y.srec}) m.add("main array", 0, *a, 8);
    put((int64_t)y.index_main * 8);
    m.add("Us", 0, y.Us, 8, kOptional); m.add("As", 0, y.As, 8, kOptional); m.add("otask (workspace)", 0, y.otask_ws, 4, kOptional);
    put((int64_t)y.main_doubles * 8);
    const size_t tb = y.tables * 8, ti = tb + T.ints * 8;   // (the table columns are relative to the table block)
    put((int64_t)tb);
    lds.add("rowmask", tb, T.rowmask, 8, kOptional, tb); lds.add("colmask", tb, T.colmask, 8, kOptional, tb); lds.add("scr", tb, T.scr, 8, kOptional, tb);
    lds.add("pushw", tb, T.pushw, 8, kOptional, tb);
    lds.add("rowpre", ti, T.rowpre, 4, kOptional, tb); lds.add("perm", ti, T.perm, 4, kOptional, tb); lds.add("boff", ti, T.boff, 4, kValue, tb); lds.add("ioff", ti, T.ioff, 4, kValue, tb);
    lds.add("lvl_col", ti, T.lvl_col, 4, kOptional, tb); lds.add("lvl_blk", ti, T.lvl_blk, 4, kOptional, tb); lds.add("lvl_mode", ti, T.lvl_mode, 4, kOptional, tb);
    lds.add("colorder", ti, T.colorder, 4, kOptional, tb); lds.add("dense_off", ti, T.dense_off, 4, kOptional, tb); lds.add("dense", ti, T.dense, 4, kOptional, tb);
    lds.add("otask", ti, T.otask, 4, kOptional, tb); lds.add("fb", ti, T.fb, 4, kOptional, tb); lds.add("last", ti, T.last, 4, kOptional, tb);
    put((int64_t)T.bytes);
    if (tb + T.bytes > lds.bytes) fail(lds.name, "the structure tables end behind the total");
    if (sp && T.ints != T.pushw.at + T.pushw.n) fail(lds.name, "the int tables do not start where the mask tables end");
    // index tables
    put(y.index_in_lds ? 1 : 0);
    Block& ix = y.index_in_lds ? s : m;
    const size_t xb = (y.index_in_lds ? y.index_lds : y.index_main) * 8;
    put((int64_t)xb);
    for (const Span* a : {&I.ilist, &I.shared, &I.r_idx, &I.p_idx, &I.s_idx}) ix.add("index table", xb, *a, 4, kValue, xb);
    put((int64_t)I.doubles * 8);
    if (y.index_in_lds != (ga && window_index_in_lds(c))) fail(lds.name, "index_in_lds is not the predicate");
    for (const Span* a : {&y.r_val, &y.p_val, &y.s_val}) lds.add("staged values", 0, *a, 8, ga ? kOptional : kValue);
    lds.add("recA", 0, Span{y.recA.at / 2, y.recA.n / 2}, 16, kOptional); lds.add("recB", 0, y.recB, 8, kOptional); lds.add("rec_count", 0, y.rec_count, 4, kOptional);
    if (y.recA.n && (y.recA.at % 2 || y.recA.n % 2)) fail(lds.name, "RecA records are not 16-byte units");
    put((int64_t)(y.recA.n ? y.recA_cap : 0));
    if (y.recA.n != 2 * y.recA_cap && !ga) fail(lds.name, "recA does not hold recA_cap records");
    lds.add("root", 0, y.root, 8, kOptional);
    put((int64_t)y.root.n * 8);
    if (y.root.n != (ga && W > 1 ? window_root_lds_doubles(c) : 0)) fail(lds.name, "root is not window_root_lds_doubles");
    put((int64_t)y.lds_bytes);
    check(m);
    if (ga) check(s);
}

template <class L>
void cov_block(const char* name, const L& l, std::initializer_list<std::pair<int, int>> dbl, std::initializer_list<std::pair<int, int>> ints) {
    Block b; b.name = name; b.bytes = l.bytes;
    for (const auto& a : dbl) b.add("double array", 0, Span{(size_t)a.first, (size_t)a.second}, 8, kSilent);
    for (const auto& a : ints) b.add("int array", (size_t)l.ints * 8, Span{(size_t)a.first, (size_t)a.second}, 4, kSilent);
    ints_follow(b, (size_t)l.ints * 8, dbl.size());
    check(b);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    int64_t head[2];
    if (!f || std::fread(head, 8, 2, f) != 2 || head[1] != 6 || head[0] < 0) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<int64_t> rows((size_t)head[0] * 6);
    if (std::fread(rows.data(), 8, rows.size(), f) != rows.size()) { std::fprintf(stderr, "%s is short\n", argv[1]); return 2; }
    std::fclose(f);
    for (g_row = 0; g_row < head[0]; ++g_row) {
        const int64_t* g = &rows[(size_t)g_row * 6];
        const WindowCaps c{(int)g[0], (int)g[2], (int)g[3], (int)g[4], (int)g[1]};
        const int nb = (int)g[5];
        wave3(c, false); wave3(c, true);
        wave6(c, false); wave6(c, true);
        arrow3(c, nb);
        window(c, false); window(c, true);
        put(window_sparse_path(c)); put(window_mask_words(c)); put((int64_t)window_nnz_capacity(c)); put(window_index_in_lds(c)); put((int64_t)window_root_lds_doubles(c));
        put(wave3_fits(c, false)); put(wave3_fits(c, true)); put(wave6_fits(c, false)); put(wave6_fits(c, true)); put(arrow3_fits(c, nb));
        put(window_fits(c, false)); put(window_fits(c, true)); put(window_arrays_in_lds(c));
        put((int64_t)(window_arrays_in_lds(c) ? window_layout(c, false).lds_bytes : window_layout(c, true).lds_bytes + 36 * sizeof(double)));   // loc_window_lds_bytes
        put(cov_chain_fits(c, false)); put(cov_chain_fits(c, true)); put(cov_forest_fits(c.nv_max, c.np_max > 0, c.ns_max > 0)); put(cov_arrow_fits(c)); put(cov_envelope_fits(c));
        const bool pr = c.np_max > 0;
        for (int d3 = 0; d3 < 2; ++d3) {
            const CovLayout l = cov_layout(c, d3 != 0);
            const bool se3 = !d3 && c.ns_max > 0;
            const int D = d3 ? 3 : 6, nv = c.nv_max;
            for (int v : {l.hd, l.ho, l.kb, l.dg, l.rrec, l.prec, l.srec, l.ints, l.ri, l.pi, l.si, l.mk}) put(v);
            put((int64_t)l.bytes);
            cov_block(d3 ? "covariance 3x3" : "covariance 6x6", l,
                      {{l.hd, nv * D * D}, {l.ho, nv * D * D}, {l.kb, D * D}, {l.dg, nv * D}, {l.rrec, kCovChunk * (1 + 2 * D)}, {l.prec, pr ? kCovChunk * 21 : 0}, {l.srec, se3 ? kCovChunk * kCovSRec : 0}},
                      {{l.ri, 2 * kCovChunk}, {l.pi, pr ? kCovChunk : 0}, {l.si, se3 ? 2 * kCovChunk : 0}, {l.mk, nv}});
        }
        {
            const int nv = c.nv_max;
            const ForestCovLayout l = forest_cov_layout(nv, pr, c.ns_max > 0);
            for (int v : {l.hd, l.ho, l.kb, l.dg, l.rec, l.ints, l.ei, l.mk, l.nd, l.ps}) put(v);
            put((int64_t)l.bytes);
            cov_block("forest covariance", l, {{l.hd, nv * 36}, {l.ho, nv * 36}, {l.kb, 36}, {l.dg, nv * 6}, {l.rec, l.ints - l.rec}}, {{l.ei, 2 * kCovChunk}, {l.mk, nv}, {l.nd, nv}, {l.ps, nv}});
        }
        {
            const int nv = c.nv_max;
            const EnvLayout l = env_layout(nv);
            for (int v : {l.sinv, l.rec, l.ints, l.ei, l.wc, l.first, l.off, l.last, l.list, l.mk}) put(v);
            put((int64_t)l.bytes);
            cov_block("envelope covariance", l, {{l.sinv, 36}, {l.rec, kEvRec}}, {{l.ei, 2 * kEvRangeChunk}, {l.wc, 4}, {l.first, nv}, {l.off, nv + 1}, {l.last, nv}, {l.list, nv}, {l.mk, nv}});
        }
        {
            const int nv = c.nv_max;
            const ArrowCovLayout l = arrow_cov_layout(nv);
            for (int v : {l.hd, l.ho, l.dg, l.cc, l.ig, l.rec, l.ints, l.ei, l.cnt, l.mk, l.flag}) put(v);
            put((int64_t)l.bytes);
            put((int64_t)arrow_cov_ws_doubles(c, nb));
            cov_block("arrowhead covariance", l, {{l.hd, nv * 9}, {l.ho, nv * 9}, {l.dg, nv * 3}, {l.cc, kAcBS * kAcBS}, {l.ig, kAcBS}, {l.rec, kAcChunk * kAcRec}},
                      {{l.ei, 2 * kAcChunk}, {l.cnt, nv}, {l.mk, nv}, {l.flag, 2}});
        }
    }
    if (g_failures) { std::fprintf(stderr, "%d failures\n", g_failures); return 1; }
    f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(g_out.data(), 8, g_out.size(), f) != g_out.size() || std::fclose(f) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    return 0;
}
