// Stand-alone driver of localization_amd/csrc/pose_records.h for tests/test_pose_records_cpu.py: built with g++ -fsanitize=address,undefined
// and run as a program.  Every array a call reads or writes is a heap array of exactly its size, so that the sanitizer sees every index.
//   records IN OUT   IN: int32 n, then n poses of 12 doubles.  OUT: n records of 7 doubles (pose_record); R_to_quat_xyzw on the 9 rotation
//                    entries alone must give the record's last four doubles, bit for bit (exit 3 otherwise)
//   gate IN OUT      IN: int32 n, then n pairs (chi2, minimum_optimize_error).  OUT: n int32
//   slots TMAX OUT   OUT: path_slot(i, nv, T) as int32 for T = 1 .. TMAX, nv = 0 .. T, i = 0 .. T - 1, in that nesting
//   windows IN OUT   one window after another — IN: int32 nv, T; double chi2, minimum_optimize_error, poison; nv poses of 12 doubles.
//                    OUT: int32 flags; realtime (7), optimized (7) as the publish step leaves poisoned rows; then for path index 0 .. T - 1:
//                    int32 present[T], rows [T][7] (absent rows keep the poison)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "pose_records.h"

namespace {

struct Reader {
    FILE* f;
    template <class T> bool maybe(T& v) { return fread(&v, sizeof(T), 1, f) == 1; }
    template <class T> T one() { T v; if (!maybe(v)) { fprintf(stderr, "short input\n"); exit(2); } return v; }
    template <class T> std::unique_ptr<T[]> many(size_t n) {   // exactly n elements on the heap
        std::unique_ptr<T[]> p(new T[n]);
        if (n && fread(p.get(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
        return p;
    }
};

FILE* open_or_die(const char* path, const char* mode) {
    FILE* f = fopen(path, mode);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    return f;
}

std::unique_ptr<double[]> filled(size_t n, double v) {
    std::unique_ptr<double[]> p(new double[n]);
    for (size_t i = 0; i < n; ++i) p[i] = v;
    return p;
}

int run_records(const char* in, const char* outp) {
    Reader rd{open_or_die(in, "rb")};
    FILE* out = open_or_die(outp, "wb");
    const int n = rd.one<int32_t>();
    for (int k = 0; k < n; ++k) {
        auto pose = rd.many<double>(12);
        std::unique_ptr<double[]> rec(new double[7]), R(new double[9]), q(new double[4]);
        locamd::pose_record(pose.get(), rec.get());
        std::memcpy(R.get(), pose.get(), 9 * sizeof(double));
        locamd::R_to_quat_xyzw(R.get(), q.get());
        if (std::memcmp(q.get(), rec.get() + 3, 4 * sizeof(double)) != 0 || std::memcmp(pose.get() + 9, rec.get(), 3 * sizeof(double)) != 0) return 3;
        fwrite(rec.get(), sizeof(double), 7, out);
    }
    fclose(out); fclose(rd.f);
    return 0;
}

int run_gate(const char* in, const char* outp) {
    Reader rd{open_or_die(in, "rb")};
    FILE* out = open_or_die(outp, "wb");
    const int n = rd.one<int32_t>();
    for (int k = 0; k < n; ++k) {
        const double chi2 = rd.one<double>(), thr = rd.one<double>();
        const int32_t g = locamd::publish_gate(chi2, thr) ? 1 : 0;
        fwrite(&g, sizeof(g), 1, out);
    }
    fclose(out); fclose(rd.f);
    return 0;
}

int run_slots(int tmax, const char* outp) {
    FILE* out = open_or_die(outp, "wb");
    for (int T = 1; T <= tmax; ++T)
        for (int nv = 0; nv <= T; ++nv)
            for (int i = 0; i < T; ++i) {
                const int32_t s = locamd::path_slot(i, nv, T);
                fwrite(&s, sizeof(s), 1, out);
            }
    fclose(out);
    return 0;
}

// one window through the rule as window_publish_kernel.hip applies it, on exactly-sized arrays
int run_windows(const char* in, const char* outp) {
    Reader rd{open_or_die(in, "rb")};
    FILE* out = open_or_die(outp, "wb");
    int32_t nv;
    while (rd.maybe(nv)) {
        const int T = rd.one<int32_t>();
        const double chi2 = rd.one<double>(), thr = rd.one<double>(), poison = rd.one<double>();
        auto poses = rd.many<double>((size_t)(nv > 0 ? nv : 0) * 12);
        auto realtime = filled(7, poison), optimized = filled(7, poison), rows = filled((size_t)T * 7, poison);
        std::unique_ptr<int32_t[]> present(new int32_t[T]);
        const bool ok = nv >= 1 && nv <= T;
        const bool pub = ok && locamd::publish_gate(chi2, thr);
        const int so = locamd::path_slot(T / 2, nv, T);
        const int32_t flags = (pub ? 1 : 0) | (ok && so >= 0 ? 2 : 0);
        if (pub) {
            locamd::pose_record(poses.get() + (size_t)(nv - 1) * 12, realtime.get());
            if (so >= 0) locamd::pose_record(poses.get() + (size_t)so * 12, optimized.get());
        }
        for (int i = 0; i < T; ++i) {
            const int s = locamd::path_slot(i, nv, T);
            present[i] = ok && s >= 0 ? 1 : 0;
            if (present[i]) locamd::pose_record(poses.get() + (size_t)s * 12, rows.get() + (size_t)i * 7);
        }
        fwrite(&flags, sizeof(flags), 1, out);
        fwrite(realtime.get(), sizeof(double), 7, out);
        fwrite(optimized.get(), sizeof(double), 7, out);
        fwrite(present.get(), sizeof(int32_t), T, out);
        fwrite(rows.get(), sizeof(double), (size_t)T * 7, out);
    }
    fclose(out); fclose(rd.f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s records|gate|slots|windows IN|TMAX OUT\n", argv[0]); return 2; }
    if (!std::strcmp(argv[1], "records")) return run_records(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "gate")) return run_gate(argv[2], argv[3]);
    if (!std::strcmp(argv[1], "slots")) return run_slots(std::atoi(argv[2]), argv[3]);
    if (!std::strcmp(argv[1], "windows")) return run_windows(argv[2], argv[3]);
    return 2;
}
