// The capture spans of sameold_amd/csrc/same_capture_dev.h compiled with a plain C++ compiler (tests/test_audio_capture_cpu.py
// builds this under ASan + UBSan): random per-channel message streams with flushes and resets are cut into random launches
// and walked launch by launch, as the transport kernel walks them; the chunks, joined, must be the captures a direct statement
// of the rule gives over the whole stream.  With a pool or a span list too small for the data, what does not fit must be marked
// and nothing may be written past either.
//
//     capture_spans_fuzz <streams> <seed>       prints one summary line, then OK
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../sameold_amd/csrc/same_capture_dev.h"

using namespace same::cap;

namespace {

struct Msg { uint64_t m; uint32_t kind; };
struct Capture {
    uint32_t channel;
    uint64_t from, to;     // to: end counter (only when the lengths are known)
    uint32_t end;          // kEnd* flag, 0 = still open at the end of the stream
    bool operator==(const Capture &o) const { return channel == o.channel && from == o.from && to == o.to && end == o.end; }
};
struct Flush { uint64_t p, z; };     // zeros fed at [p, p + z)
struct Reset { uint64_t r; std::vector<uint32_t> chans; };

int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); ++g_fail; return; } } while (0)

// the rule over the whole stream (include/same_rx.h): per channel, its messages, flush starts and resets in stream order
std::vector<Capture> reference(uint32_t n_ch, const std::vector<std::vector<Msg>> &msgs, const std::vector<Flush> &flushes,
                               const std::vector<Reset> &resets)
{
    std::vector<Capture> out;
    for (uint32_t c = 0; c < n_ch; ++c) {
        struct Ev { uint64_t pos; int type; uint32_t kind; };      // type 0 message, 1 reset, 2 flush start
        std::vector<Ev> ev;
        for (const Msg &m : msgs[c]) ev.push_back({m.m, 0, m.kind});
        for (const Reset &r : resets)
            if (std::find(r.chans.begin(), r.chans.end(), c) != r.chans.end()) ev.push_back({r.r, 1, 0});
        for (const Flush &f : flushes) ev.push_back({f.p, 2, 0});
        std::stable_sort(ev.begin(), ev.end(), [](const Ev &a, const Ev &b) { return a.pos != b.pos ? a.pos < b.pos : a.type < b.type; });
        bool open = false;
        uint64_t from = 0;
        for (const Ev &e : ev) {
            if (e.type == 1 || e.type == 2) {
                if (open) out.push_back({c, from, e.pos, e.type == 1 ? kEndReset : kEndFlush});
                open = false;
                continue;
            }
            bool in_flush = false;
            for (const Flush &f : flushes) in_flush |= e.pos > f.p && e.pos <= f.p + f.z;
            if (in_flush) {
                if (e.kind == kMsgStart) out.push_back({c, e.pos, e.pos, kEndFlush});
                continue;
            }
            if (open) out.push_back({c, from, e.pos, kEndMessage});
            open = false;
            if (e.kind == kMsgStart) { open = true; from = e.pos; }
        }
        if (open) out.push_back({c, from, 0, 0});
    }
    return out;
}

struct Stats { uint64_t streams = 0, launches = 0, captures = 0, chunks = 0, truncated = 0, lost_spans = 0; } g_stats;

void run_stream(std::mt19937_64 &rng, bool tight)
{
    auto uni = [&](uint64_t lo, uint64_t hi) { return std::uniform_int_distribution<uint64_t>(lo, hi)(rng); };
    const uint32_t n_ch = (uint32_t)uni(1, 4);
    // the stream: real samples with flushes (zeros) in between; resets between calls
    std::vector<Flush> flushes;
    std::vector<uint64_t> cuts{0};          // launch boundaries that every cutting must have
    uint64_t T = 0;
    const int n_seg = (int)uni(1, 4);
    for (int s = 0; s < n_seg; ++s) {
        T += uni(1, 400);
        if (uni(0, 2) == 0) {
            const uint64_t z = uni(1, 200);
            flushes.push_back({T, z});
            T += z;
            cuts.push_back(T);              // the next call's launches begin behind the flush
        }
    }
    auto in_flush_open = [&](uint64_t p) { for (const Flush &f : flushes) if (p > f.p && p < f.p + f.z) return true; return false; };
    std::vector<Reset> resets;
    for (int k = (int)uni(0, 3); k > 0; --k) {
        if (T < 2) break;
        const uint64_t r = uni(1, T - 1);      // (between two calls: a launch begins there)
        if (in_flush_open(r)) continue;
        Reset rs{r, {}};
        for (uint32_t c = 0; c < n_ch; ++c) if (uni(0, 1)) rs.chans.push_back(c);
        bool dup = false;
        for (const Reset &o : resets) dup |= o.r == r;
        if (dup) continue;
        resets.push_back(rs);
        cuts.push_back(r);
    }
    // flush starts: a launch boundary in ordinary batches; under SAME_BATCH_CALL_INVARIANT a window may hold both sides
    for (const Flush &f : flushes) if (uni(0, 1)) cuts.push_back(f.p);
    for (int k = (int)uni(0, 12); k > 0; --k) cuts.push_back(uni(1, T));
    cuts.push_back(T);
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    // messages: counters in (0, T], several on one counter now and then
    std::vector<std::vector<Msg>> msgs(n_ch);
    for (uint32_t c = 0; c < n_ch; ++c) {
        const int k = (int)uni(0, 12);
        for (int i = 0; i < k; ++i) msgs[c].push_back({uni(1, T), uni(0, 2) ? kMsgStart : kMsgEnd});
        std::stable_sort(msgs[c].begin(), msgs[c].end(), [](const Msg &a, const Msg &b) { return a.m < b.m; });
    }

    const uint64_t pool_cap = tight ? uni(0, 60) : 1u << 20;
    const bool small_list = tight && uni(0, 1);
    std::vector<Rec> rec(n_ch, Rec{0, 0, 0});
    std::vector<uint8_t> host_open(n_ch, 0);
    struct Chunk { uint32_t channel, flags; uint64_t counter, n; };
    std::vector<Chunk> chunks;
    uint64_t lost = 0;
    for (size_t li = 0; li + 1 < cuts.size(); ++li) {
        const uint64_t S = cuts[li], E = cuts[li + 1];
        // resets at S: the host ends the open captures (from the chunks it has), the reset kernel closes the device records
        for (const Reset &r : resets)
            if (r.r == S)
                for (uint32_t c : r.chans) {
                    if (host_open[c]) { chunks.push_back({c, kEndReset, S, 0}); host_open[c] = 0; }
                    rec[c] = Rec{0, 0, 0};
                }
        uint64_t fa = UINT64_MAX;
        for (const Flush &f : flushes) if (S < f.p + f.z && f.p < E) fa = f.p;
        const uint32_t n_rows = (uint32_t)(E - S);
        const uint32_t span_cap = tight && small_list ? (uint32_t)uni(0, 4) : n_ch * 16 + 8;
        std::vector<Span> spans(span_cap);                 // exactly this many: ASan catches a write past it
        Cursors cur{0, 0, 0};
        Launch L{};
        L.start = S; L.n_rows = n_rows;
        L.flush_row = fa >= E ? kNoFlush : (uint32_t)(fa > S ? fa - S : 0);
        L.rec = rec.data(); L.spans = spans.data(); L.span_cap = span_cap;
        L.n_spans = &cur.n_spans; L.pool_used = &cur.pool_used; L.pool_cap = pool_cap; L.overflow = &cur.overflow;
        for (uint32_t c = 0; c < n_ch; ++c) {
            Walker w(L, c);
            for (const Msg &m : msgs[c]) if (m.m > S && m.m <= E) w.on_message(m.kind, m.m);
            w.finish();
        }
        ++g_stats.launches;
        // what the capture kernel and the harvest would do with the list
        const uint32_t n_spans = std::min(cur.n_spans, span_cap);
        if (cur.n_spans > span_cap) { CHECK(cur.overflow & kAudioOverflow, "lost spans not flagged"); lost += cur.n_spans - span_cap; }
        std::vector<std::pair<uint64_t, uint64_t>> used;
        bool any_trunc = false;
        for (uint32_t i = 0; i < n_spans; ++i) {
            const Span &s = spans[i];
            CHECK(s.channel < n_ch, "channel");
            CHECK(s.counter == S + s.row0, "counter %llu, row %u of a launch at %llu", (unsigned long long)s.counter, s.row0, (unsigned long long)S);
            CHECK(s.row0 <= n_rows && s.n <= n_rows - s.row0, "span past the launch");
            CHECK(s.n == 0 || (s.off <= pool_cap && s.n <= pool_cap - s.off), "span past the pool");
            if (L.flush_row != kNoFlush) CHECK(s.row0 + s.n <= L.flush_row || s.n == 0, "a flush row was captured");
            if (s.n) used.push_back({s.off, s.off + s.n});
            any_trunc |= (s.flags & kTruncated) != 0;
        }
        std::sort(used.begin(), used.end());
        for (size_t i = 1; i < used.size(); ++i) CHECK(used[i].first >= used[i - 1].second, "pool ranges overlap");
        if (any_trunc) { CHECK(cur.overflow & kAudioOverflow, "truncation not flagged"); ++g_stats.truncated; }
        if (!tight) CHECK(!cur.overflow, "overflow with room to spare");
        std::vector<uint32_t> order(n_spans);
        for (uint32_t i = 0; i < n_spans; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return spans[a].channel < spans[b].channel; });
        for (uint32_t i : order) {
            const Span &s = spans[i];
            chunks.push_back({s.channel, s.flags, s.counter, s.n});
            if (s.flags & kFirst) host_open[s.channel] = 1;
            if (s.flags & (kEndMessage | kEndFlush | kEndReset)) host_open[s.channel] = 0;
        }
    }
    g_stats.chunks += chunks.size();
    g_stats.lost_spans += lost;
    ++g_stats.streams;
    // lost span records can lose a capture's FIRST or END chunk: only what was delivered was checked
    if (lost) return;

    // join the chunks per channel (in queue order) into captures
    std::vector<Capture> got;
    std::vector<int> open_at(n_ch, -1);
    std::vector<bool> trunc(n_ch, false);
    for (const Chunk &k : chunks) {
        if (k.flags & kFirst) {
            CHECK(open_at[k.channel] < 0, "channel %u: FIRST at %llu inside a capture", k.channel, (unsigned long long)k.counter);
            open_at[k.channel] = (int)got.size();
            got.push_back({k.channel, k.counter, k.counter, 0});
            trunc[k.channel] = false;
        }
        CHECK(open_at[k.channel] >= 0, "channel %u: chunk at %llu outside any capture", k.channel, (unsigned long long)k.counter);
        Capture &cp = got[(size_t)open_at[k.channel]];
        if (!tight) {
            CHECK(!(k.flags & kTruncated), "truncated with room to spare");
            CHECK(k.counter == cp.to, "channel %u: chunk at %llu, the capture had reached %llu", k.channel, (unsigned long long)k.counter,
                  (unsigned long long)cp.to);
            cp.to = k.counter + k.n;
        } else {
            cp.to = 0;      // (lengths unknown once a chunk was cut short)
        }
        if (k.flags & (kEndMessage | kEndFlush | kEndReset)) {
            cp.end = k.flags & (kEndMessage | kEndFlush | kEndReset);
            open_at[k.channel] = -1;
        }
    }
    for (Capture &cp : got) if (cp.end == 0) cp.to = 0;
    std::vector<Capture> want = reference(n_ch, msgs, flushes, resets);
    if (tight) for (Capture &cp : want) cp.to = 0;
    auto key = [](const Capture &a, const Capture &b) { return a.channel != b.channel ? a.channel < b.channel : a.from < b.from; };
    std::stable_sort(got.begin(), got.end(), key);
    std::stable_sort(want.begin(), want.end(), key);
    CHECK(got.size() == want.size(), "%zu captures, the rule gives %zu", got.size(), want.size());
    for (size_t i = 0; i < got.size(); ++i)
        CHECK(got[i] == want[i], "capture %zu: ch %u [%llu, %llu) end %u, the rule: ch %u [%llu, %llu) end %u", i, got[i].channel,
              (unsigned long long)got[i].from, (unsigned long long)got[i].to, got[i].end, want[i].channel, (unsigned long long)want[i].from,
              (unsigned long long)want[i].to, want[i].end);
    g_stats.captures += got.size();
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s <streams> <seed>\n", argv[0]); return 2; }
    const long n = std::atol(argv[1]);
    std::mt19937_64 rng((uint64_t)std::atoll(argv[2]));
    for (long i = 0; i < n && !g_fail; ++i) run_stream(rng, i % 4 == 3);
    if (g_fail) return 1;
    std::printf("%llu streams %llu launches %llu captures %llu chunks %llu truncated %llu lost equal\n", (unsigned long long)g_stats.streams,
                (unsigned long long)g_stats.launches, (unsigned long long)g_stats.captures, (unsigned long long)g_stats.chunks,
                (unsigned long long)g_stats.truncated, (unsigned long long)g_stats.lost_spans);
    std::printf("OK\n");
    return 0;
}
