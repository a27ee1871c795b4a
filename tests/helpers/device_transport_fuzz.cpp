// The device transport layer (sameold_amd/csrc/same_transport_dev.h) built as plain C++, against the host's same::TransportRef.
//
//   device_transport_fuzz golden <events.txt>   replay "kind sample symbol hex|-" lines through same::dt::Transport and print
//                                               every transport event as "kind sample len text"
//   device_transport_fuzz fuzz <streams> <seed> random per-channel streams through both; any difference fails
//
// Built with -fsanitize=address,undefined by tests/test_device_transport_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sameold_amd/csrc/same_transport.h"
#include "../../sameold_amd/csrc/same_transport_dev.h"

static int hexval(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

static int golden(const char *path)
{
    FILE *f = std::fopen(path, "r");
    if (!f) { std::perror(path); return 2; }
    same::dt::Hot h{};
    same::dt::Cold *c = new same::dt::Cold;
    same::dt::Transport tr{h, *c};
    tr.reset();
    same::dt::Msg msg;
    same::dt::Event ev;
    char hex[1024];
    unsigned kind; unsigned long long sc, sym;
    while (std::fscanf(f, "%u %llu %llu %1023s", &kind, &sc, &sym, hex) == 4) {
        std::vector<uint8_t> bytes;
        if (hex[0] != '-') for (size_t i = 0; hex[i] && hex[i + 1]; i += 2) bytes.push_back((uint8_t)(hexval(hex[i]) * 16 + hexval(hex[i + 1])));
        const uint32_t n = bytes.size() < SAME_EVENT_MAX_BYTES ? (uint32_t)bytes.size() : SAME_EVENT_MAX_BYTES;
        if (tr.on_link_event(kind, sc, sym, bytes.data(), n, 22050, msg, &ev)) {
            std::printf("%u %" PRIu64 " %u ", ev.kind, ev.sample_counter, ev.len);
            if (ev.kind == SAME_TRANSPORT_MSG_START) std::fwrite(ev.text, 1, ev.len, stdout);
            std::printf("\n");
        }
        (void)tr.force_eom_dirty();
    }
    std::fclose(f);
    delete c;
    std::printf("OK\n");
    return 0;
}

// ---- random streams -------------------------------------------------------------------------------------------------
struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
    bool chance(uint32_t pct) { return below(100) < pct; }
};

static const char *const kTexts[] = {
    "ZCZC-WXR-TOR-029037+0030-1051700-KEAX/NWS-",
    "ZCZC-WXR-SVR-029037-029038-029039+0100-1051715-KEAX/NWS-",
    "ZCZC-EAS-RWT-012057-012081-012101-012103-012115+0100-3471200-WAGA/TV-",
    "ZCZC-CIV-CAE-000000+0015-0010000-ABC-",
    "ZCZC-PEP-EAN-000000+0400-1231159-WHITE/HS-",
    "ZCZC-WXR-TOR-029037+0030-1051700-KEAX/NWS",        // no final dash: Malformed
    "ZCZC-WX1-TOR-029037+0030-1051700-KEAX/NWS-",       // Malformed
    "NNNN",
    "NNNNNNNN",
    "NN",
    "XYZZY-hello world",
};

static void make_burst(Rng &r, std::vector<uint8_t> &b)
{
    const char *t = kTexts[r.below(sizeof(kTexts) / sizeof(kTexts[0]))];
    b.assign(t, t + std::strlen(t));
    // ragged lengths: trailing garbage (often 0xab filler or a character not allowed), truncation, or a long tail
    const uint32_t tail = r.chance(30) ? r.below(8) : (r.chance(5) ? 200 + r.below(100) : 0);
    for (uint32_t i = 0; i < tail; ++i) b.push_back(r.chance(50) ? 0xabu : (uint8_t)r.below(256));
    if (r.chance(15) && !b.empty()) b.resize(r.below((uint32_t)b.size() + 1));
    // bit errors and high bits
    const uint32_t flips = r.chance(50) ? 0 : r.below(4);
    for (uint32_t i = 0; i < flips && !b.empty(); ++i) b[r.below((uint32_t)b.size())] ^= (uint8_t)(1u << r.below(8));
    if (r.chance(10) && !b.empty()) b[r.below((uint32_t)b.size())] |= 0x80u;
    if (b.size() > SAME_EVENT_MAX_BYTES) b.resize(SAME_EVENT_MAX_BYTES);
}

static bool same_event(const same_rx_event &a, const same::dt::Event &b)
{
    if (a.kind != b.kind || a.sample_counter != b.sample_counter || a.symbol_count != b.symbol_count || a.len != b.len ||
        a.aux != b.aux || a.aux2 != b.aux2) return false;
    if (a.kind == SAME_TRANSPORT_MSG_START) return b.text && std::memcmp(a.bytes, b.text, a.len) == 0;
    return true;
}

static int fuzz(long n_streams, uint64_t seed)
{
    Rng r{seed};
    same::TransportHot *rh = new same::TransportHot;
    same::TransportCold *rc = new same::TransportCold;
    same::dt::Hot dh{};
    same::dt::Cold *dc = new same::dt::Cold;
    std::vector<uint8_t> burst;
    long events = 0, messages = 0, forced = 0;
    const uint32_t rates[] = {22050, 48000, 8, 1};
    for (long s = 0; s < n_streams; ++s) {
        same::TransportRef ref(*rh, *rc);
        same::dt::Transport dev{dh, *dc};
        ref.reset(); dev.reset();
        // a small input rate brings the 135-second forced end of message within a few thousand samples
        const uint32_t rate = rates[r.below(4)];
        const double sps = rate >= 8000 ? rate / 520.83 : 1.0 + r.below(40);
        uint64_t sym = r.below(1000), t = (uint64_t)(sym * sps) + r.below(50);
        const uint32_t n_ev = 10 + r.below(50);
        std::vector<uint64_t> deadlines;
        for (uint32_t e = 0; e < n_ev; ++e) {
            uint32_t kind;
            const uint32_t pick = r.below(100);
            // the next instant: a few symbols on, on or beside a deadline a burst armed, or far on
            uint64_t step;
            if (pick < 35 && !deadlines.empty()) {
                const uint64_t d = deadlines[r.below((uint32_t)deadlines.size())] + r.below(3) - 1;
                step = d > sym ? d - sym : 1 + r.below(3);
            } else if (pick < 45) {
                step = 600 + r.below(6000);
            } else {
                step = 1 + r.below(200);
            }
            if (r.chance(3)) step = 0;                    // a second event on the same symbol
            sym += step; t += (uint64_t)(step * sps) + r.below(3);
            const uint32_t k = r.below(100);
            if (k < 30) kind = SAME_LINK_BURST;
            else if (k < 50) kind = SAME_LINK_NO_CARRIER;
            else if (k < 90) kind = same::kDevTick;
            else if (k < 95) kind = SAME_LINK_SEARCHING;
            else kind = SAME_LINK_READING;
            // a wake-up right after the forced-EOM instant, as the device makes one
            if (kind == same::kDevTick && ref.force_eom_at() && r.chance(40) && ref.force_eom_at() + 1 > t) {
                t = ref.force_eom_at() + 1 + r.below(2);
                ++forced;
            }
            const uint8_t *bytes = nullptr;
            uint32_t len = 0;
            if (kind == SAME_LINK_BURST) {
                make_burst(r, burst);
                if (!r.chance(3)) { bytes = burst.data(); len = (uint32_t)burst.size(); }      // (else: a burst the pool lost)
                deadlines.push_back(sym + same::max_interburst_symbols());
                deadlines.push_back(sym + same::max_history_duration());
            }
            same_rx_event a;
            std::memset(&a, 0, sizeof(a));
            same::dt::Msg msg;
            same::dt::Event b{};
            const bool ga = ref.on_link_event(kind, t, sym, bytes, len, rate, &a);
            const bool gb = dev.on_link_event(kind, t, sym, bytes, len, rate, msg, &b);
            ++events;
            if (ga != gb || (ga && !same_event(a, b))) {
                std::printf("stream %ld event %u (kind %u sample %" PRIu64 " symbol %" PRIu64 " len %u): reference %d kind %u len %u aux %u/%u, "
                            "device %d kind %u len %u aux %u/%u\n", s, e, kind, t, sym, len, ga, a.kind, a.len, a.aux, a.aux2, gb, b.kind,
                            b.len, b.aux, b.aux2);
                return 1;
            }
            if (ga && a.kind >= SAME_TRANSPORT_MSG_START) ++messages;
            if (ref.force_eom_at() != dev.force_eom_at() || ref.force_eom_dirty() != dev.force_eom_dirty()) {
                std::printf("stream %ld event %u: forced-EOM instant differs\n", s, e);
                return 1;
            }
        }
    }
    delete rh; delete rc; delete dc;
    std::printf("%ld streams, %ld events, %ld transport messages, %ld forced-EOM wake-ups: equal\n", n_streams, events, messages, forced);
    std::printf("OK\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (same::dt::kMaxInterburstSymbols != same::max_interburst_symbols() || same::dt::kMaxHistoryDuration != same::max_history_duration()) {
        std::printf("assembler constants differ\n");
        return 1;
    }
    if (argc > 2 && std::strcmp(argv[1], "golden") == 0) return golden(argv[2]);
    if (argc > 3 && std::strcmp(argv[1], "fuzz") == 0) return fuzz(std::atol(argv[2]), std::strtoull(argv[3], nullptr, 10));
    std::fprintf(stderr, "usage: %s golden <events.txt> | fuzz <streams> <seed>\n", argv[0]);
    return 2;
}
