// The staging tables of the host-pointer entries (csrc/hmpc_stage.h) without a GPU, built with g++ -fsanitize=address,undefined.
// Every table is built by the function the library calls.  The "device" is a second heap block of exactly `total` bytes and the
// two transfers are memcpy over the ranges the library copies ([0, in_end) up, [out_begin, total) down, or part by part), so an
// offset one byte too far is a sanitizer report.  Checked per table: offsets are multiples of 256, parts lie back to back in
// order (no overlap, `total` minimal), an absent part has no room and a null pointer, the outputs begin where the last input
// ends; pack -> the device writes a pattern into every output -> unpack carries every byte of every present part and touches
// nothing behind the caller's arrays (guard bytes).  Prints the solve table's offsets as JSON lines for tests/test_stage_host.py.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "hmpc_stage.h"

static int failures = 0;
#define CHECK(cond, ...)                                                                                     \
    do {                                                                                                     \
        if (!(cond)) { failures++; fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } \
    } while (0)

constexpr size_t GUARD = 32;
constexpr unsigned char GUARD_BYTE = 0xA5, UNTOUCHED = 0xEE;

// a caller's array of n bytes with guard bytes behind it: inputs hold a pattern, outputs UNTOUCHED
struct Arr {
    std::vector<unsigned char> v;
    size_t n;
    Arr(size_t n_, bool input, unsigned seed) : v(n_ + GUARD, GUARD_BYTE), n(n_)
    {
        for (size_t i = 0; i < n; i++) v[i] = input ? (unsigned char)(seed * 31 + i * 7 + (i >> 8)) : UNTOUCHED;
    }
    template <class T> T *p() { return (T *)v.data(); }
    bool guard_ok() const
    {
        for (size_t i = n; i < n + GUARD; i++)
            if (v[i] != GUARD_BYTE) return false;
        return true;
    }
};
static std::vector<std::unique_ptr<Arr>> arrays;
template <class T> static T *arr(size_t bytes, bool input, bool wanted = true)
{
    if (!wanted) return nullptr;
    arrays.emplace_back(new Arr(bytes, input, (unsigned)arrays.size() + 1));
    return arrays.back()->p<T>();
}
static void check_guards(const char *what)
{
    for (const auto &a : arrays) CHECK(a->guard_ok(), "%s: bytes behind a caller's array of %zu bytes were written", what, a->n);
    arrays.clear();
}

static size_t up(size_t v) { return (v + 255) / 256 * 256; }
static unsigned char device_byte(int part, size_t j) { return (unsigned char)(0x40 + part * 13 + j * 3 + (j >> 7)); }

static void check_layout(const StageTable &t, const char *what)
{
    size_t at = 0;
    char *const base = (char *)4096; // (ptr only adds an offset)
    for (int i = 0; i < t.n; i++) {
        const StagePart &p = t.part[i];
        CHECK(p.off % 256 == 0, "%s part %d at %zu", what, i, p.off);
        CHECK(p.off == at, "%s part %d at %zu, the parts before it end at %zu", what, i, p.off, at);
        at += up(p.bytes + p.pad);
        CHECK((t.ptr<char>(i, base) == nullptr) == (p.bytes == 0), "%s part %d: a null pointer exactly where there are no bytes", what, i);
        if (p.bytes) CHECK(t.ptr<char>(i, base) == base + p.off, "%s part %d", what, i);
        CHECK(i >= t.n_in || !p.dst, "%s part %d: an input with a destination", what, i);
        CHECK(i < t.n_in || p.dst || !p.src, "%s part %d", what, i);
    }
    CHECK(t.total == at, "%s total %zu, the parts need %zu", what, t.total, at);
    CHECK(t.n_in <= t.n, "%s", what);
    const size_t first_out = t.n_in < t.n ? t.part[t.n_in].off : t.total;
    CHECK(t.out_begin == first_out, "%s out_begin %zu, the last input ends at %zu", what, t.out_begin, first_out);
    const bool both = t.n_in < t.n && t.part[t.n_in].src;
    CHECK(t.in_end == (both ? first_out + up(t.part[t.n_in].bytes) : first_out), "%s in_end %zu", what, t.in_end);
    for (int i = t.n_in + 1; i < t.n; i++) CHECK(!t.part[i].src, "%s part %d: only the first part that comes down may travel up", what, i);
}

// pack, copy up, the device writes every output, copy down, unpack (`rows`: of the parts from `rows_from` on); `each`: part by
// part between the caller's arrays and the device block (the shift and the search entries), without a host block
static void round_trip(const StageTable &t, const char *what, bool each = false, int rows_from = 1 << 30, size_t rows = SIZE_MAX)
{
    std::unique_ptr<char[]> host(new char[t.total ? t.total : 1]), dev(new char[t.total ? t.total : 1]);
    memset(host.get(), 0x11, t.total);
    memset(dev.get(), 0x22, t.total);
    if (each) {
        for (int i = 0; i < t.n_in; i++)
            if (t.part[i].bytes && t.part[i].src) memcpy(dev.get() + t.part[i].off, t.part[i].src, t.part[i].bytes);
    } else {
        t.pack(host.get());
        memcpy(dev.get(), host.get(), t.in_end);
    }
    for (int i = 0; i < t.n; i++) { // what the device reads is what the caller holds
        const StagePart &p = t.part[i];
        if (!p.src || !p.bytes) continue;
        const char *d = t.ptr<char>(i, dev.get());
        const size_t row = p.row ? p.row : p.bytes, stride = p.row ? p.stride : 0;
        for (size_t r = 0; r * row < p.bytes; r++)
            CHECK(memcmp(d + r * row, (const char *)p.src + r * stride, row) == 0, "%s part %d row %zu did not arrive", what, i, r);
    }
    for (int i = t.n_in; i < t.n; i++)
        if (unsigned char *d = t.ptr<unsigned char>(i, dev.get()))
            for (size_t j = 0; j < t.part[i].bytes; j++) d[j] = device_byte(i, j);
    for (int i = t.n_in; i < t.n; i++) {
        const StagePart &p = t.part[i];
        const size_t r = i >= rows_from ? rows : SIZE_MAX;
        if (each) {
            if (p.bytes && p.dst) memcpy(p.dst, dev.get() + p.off, p.bytes);
        } else {
            if (i == t.n_in && t.total > t.out_begin) memcpy(host.get() + t.out_begin, dev.get() + t.out_begin, t.total - t.out_begin);
            t.unpack(host.get(), i, r);
        }
        if (!p.dst || !p.bytes) continue;
        const size_t got = p.row && r < p.bytes / p.row ? r * p.row : p.bytes;
        const unsigned char *d = (const unsigned char *)p.dst;
        for (size_t j = 0; j < p.bytes; j++)
            if (d[j] != (j < got ? device_byte(i, j) : UNTOUCHED)) { CHECK(false, "%s part %d byte %zu of %zu (%zu asked for)", what, i, j, p.bytes, got); break; }
    }
    check_guards(what);
}

static void solve_cases(const StageDims &d)
{
    const size_t Bs[] = {1, 7, 63, 64, 65, 300};
    for (size_t B : Bs)
        for (size_t nwarm : {(size_t)0, (size_t)1, B})
            for (size_t stride : {(size_t)0, d.nx, d.nx + 3})
                for (int ask = 0; ask < 3; ask++) { // nothing but the small outputs / primal / primal and dual
                    const size_t xn = (stride ? (B - 1) * stride : 0) + d.nx;
                    const double *x0 = arr<double>(xn * sizeof(double), true);
                    const int8_t *fix = arr<int8_t>(B * d.nfix, true);
                    const hmpc_result out{arr<double>(B * 8, false), arr<double>(B * 8, false, ask != 1), arr<int32_t>(B * 4, false), arr<int32_t>(B * 4, false, ask != 2),
                                          arr<double>(B * d.n_primal * 8, false, ask >= 1), arr<double>(B * d.n_dual * 8, false, ask == 2)};
                    const StageTable t = stage_solve(d, B, nwarm, x0, stride, fix, &out);
                    check_layout(t, "solve");
                    CHECK(t.n == SOLVE_DUAL + 1 && t.n_in == SOLVE_OBJ, "solve: %d parts, %d inputs", t.n, t.n_in);
                    // the capacity's table (no arrays) has this batch's offsets: the room of a part does not depend on what is asked for
                    const StageTable cap = stage_solve(d, B, nwarm, nullptr, 0, nullptr, nullptr);
                    for (int i = 0; i < t.n; i++) CHECK(cap.part[i].off == t.part[i].off, "solve part %d", i);
                    CHECK(cap.total == t.total, "solve");
                    {   // x0 packs as the parent's loop does: one row for stride 0, else B rows of nx doubles read `stride` doubles apart
                        std::vector<char> block(t.total, 0), want(B * d.nx * sizeof(double), 0);
                        t.pack(block.data());
                        if (stride == 0) memcpy(want.data(), x0, d.nx * sizeof(double));
                        else
                            for (size_t b = 0; b < B; b++) memcpy(want.data() + b * d.nx * sizeof(double), x0 + b * stride, d.nx * sizeof(double));
                        CHECK(memcmp(block.data() + t.part[SOLVE_X0].off, want.data(), (stride ? B : 1) * d.nx * sizeof(double)) == 0, "solve x0 stride %zu", stride);
                        CHECK(memcmp(block.data() + t.part[SOLVE_FIX].off, fix, B * d.nfix) == 0, "solve fix");
                    }
                    if (ask == 0 && stride == 0) {
                        printf("{\"nx\": %zu, \"nfix\": %zu, \"n_primal\": %zu, \"n_dual\": %zu, \"B\": %zu, \"nwarm\": %zu, \"off\": [", d.nx, d.nfix, d.n_primal, d.n_dual, B, nwarm);
                        for (int i = 0; i < t.n; i++) printf("%zu, ", t.part[i].off);
                        printf("%zu, %zu]}\n", t.in_end, t.total);
                    }
                    round_trip(t, "solve");
                }
}

static void certify_cases(const StageDims &d)
{
    for (size_t B : {(size_t)1, (size_t)130})
        for (size_t stride : {(size_t)0, d.nx, d.nx + 3})
            for (bool verdict : {false, true}) {
                const hmpc_result rec{arr<double>(B * 8, true), arr<double>(B * 8, true), arr<int32_t>(B * 4, true), arr<int32_t>(B * 4, true),
                                      arr<double>(B * d.n_primal * 8, true), arr<double>(B * d.n_dual * 8, true)};
                const StageTable t = stage_certify(d, B, arr<double>(((stride ? (B - 1) * stride : 0) + d.nx) * 8, true), stride, arr<int8_t>(B * d.nfix, true), rec,
                                                   arr<double>(B * HMPC_CERT_COUNT * 8, false), arr<int32_t>(B * 4, false, verdict));
                check_layout(t, "certify");
                CHECK(t.n == CERT_VERDICT + 1 && t.n_in == CERT_RES, "certify: %d parts, %d inputs", t.n, t.n_in);
                round_trip(t, "certify");
            }
}

static void branch_cases(const StageDims &d)
{
    for (size_t B : {(size_t)1, (size_t)7})
        for (int ask = 0; ask < 4; ask++) // n_children alone / everything with cutoff and mark_weak / everything without / the digest only
            for (size_t nchild : {(size_t)0, (size_t)1, 2 * B}) {
                const bool all = ask == 1 || ask == 2, dig = all || ask == 3, weak = ask == 1;
                const hmpc_result rec{arr<double>(B * 8, true), arr<double>(B * 8, true), arr<int32_t>(B * 4, true), arr<int32_t>(B * 4, true),
                                      arr<double>(B * d.n_primal * 8, true), arr<double>(B * d.n_dual * 8, true)};
                const hmpc_branch_out out{arr<double>(B * 8, false, dig), arr<int32_t>(B * 4, false, dig), arr<int32_t>(B * 4, false, dig), arr<double>(2 * B * 8, false, dig),
                                          arr<uint64_t>(B * d.words * 8, false, dig), arr<int32_t>(B * 4, false, all), arr<int32_t>(4, false, ask != 3),
                                          arr<int8_t>(2 * B * d.nfix, false, all), arr<double>(2 * B * 8, false, all), arr<int32_t>(2 * B * 4, false, all),
                                          arr<int32_t>(2 * B * 4, false, all)};
                const StageTable t = stage_branch(d, B, arr<int8_t>(B * d.nfix, true), rec, arr<double>(B * 8, true, weak), weak, out);
                check_layout(t, "branch");
                CHECK(t.n == BR_O_CWARM + 1 && t.n_in == BR_DOBJ, "branch: %d parts, %d inputs", t.n, t.n_in);
                CHECK((t.part[BR_DOBJ].bytes != 0) == weak && (t.part[BR_CUTOFF].bytes != 0) == weak, "branch: dual objectives and cutoff travel only where asked for");
                CHECK((t.part[BR_PRIMAL].bytes != 0) == dig && (t.part[BR_DUAL].bytes != 0) == dig, "branch: the records' rows travel only where an output needs them");
                if (ask == 0) CHECK(t.total - t.out_begin == 256, "branch: n_children alone is one part of the copy down");
                round_trip(t, "branch", false, BR_O_CFIX, nchild); // the child arrays stop at n_children rows
            }
}

static void shift_and_search_cases(const StageDims &d)
{
    const size_t B = 5, K = 2;
    StageTable t = stage_shift(d, B, K, arr<int32_t>(B * 4, true), arr<double>(K * d.nx * 8, true), arr<double>(K * d.nu * 8, true), arr<double>(K * d.nx * 8, true),
                               arr<int8_t>(B * d.nfix, true), arr<double>(B * 8, true), arr<double>(B * d.n_dual * 8, true), arr<double>(B * 8, true),
                               arr<int8_t>(B * d.nfix, false), arr<double>(B * 8, false), arr<double>(B * d.n_dual * 8, false), arr<double>(B * 8, false), arr<uint8_t>(B, false));
    check_layout(t, "shift");
    CHECK(t.n == SH_O_FLAGS + 1 && t.n_in == SH_O_FIX, "shift: %d parts, %d inputs", t.n, t.n_in);
    round_trip(t, "shift", true);
    for (size_t total : {(size_t)0, (size_t)5}) {
        t = stage_search_begin(d, K, total, arr<int32_t>((K + 1) * 4, true), arr<int8_t>(total * d.nfix, true), arr<double>(total * 8, true));
        check_layout(t, "search_begin");
        CHECK(t.n == 3 && t.n_in == 3 && t.out_begin == t.total, "search_begin: inputs only");
        round_trip(t, "search_begin", true);
    }
    for (int ask = 0; ask < 3; ask++) { // everything / the leaves' numbers alone (hmpc_search_leaves) / nothing
        const bool all = ask == 0;
        t = stage_search_results(d, K, arr<double>(K * 8, false, all), arr<double>(K * d.nu * 8, false, all), arr<double>(K * d.nx * 8, false, all),
                                 arr<int8_t>(K * d.nfix, false, all), arr<int32_t>(K * 4, false, all), arr<int32_t>(K * 4, false, ask < 2), arr<int32_t>(K * 4, false, all),
                                 arr<int32_t>(K * 4, false, all));
        check_layout(t, "search_results");
        CHECK(t.n == 8 && t.n_in == 0 && t.out_begin == 0 && (t.total == 0) == (ask == 2), "search_results: outputs only");
        round_trip(t, "search_results", true);
    }
    for (bool all : {true, false}) {
        const size_t N = 3;
        t = stage_search_leaves(d, K, N, arr<int32_t>(K * 4, true), arr<int32_t>(N * 4, false), arr<int8_t>(N * d.nfix, false, all), arr<double>(N * 8, false),
                                arr<double>(N * d.n_dual * 8, false, all), arr<double>(N * 8, false, all), arr<uint8_t>(N, false, all));
        check_layout(t, "search_leaves");
        CHECK(t.n == 7 && t.n_in == 1, "search_leaves");
        round_trip(t, "search_leaves", true);
    }
}

int main()
{
    // the cart-pole with walls at T = 10 (nx 4, nu 7, nub 4), and an odd shape (nx 3, nu 2, nub 1, T 3; an odd dual row)
    const StageDims shapes[] = {{4, 7, 40, 1, 114, 560}, {3, 2, 3, 1, 18, 37}};
    for (const StageDims &d : shapes) {
        solve_cases(d);
        certify_cases(d);
        branch_cases(d);
        shift_and_search_cases(d);
    }
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    return 0;
}
