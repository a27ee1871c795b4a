// same_harvest.cpp -- the host half of a harvest (same_harvest.h): event queue, audio queue, the replay of a launch's ordered
// log (ordering, time-parallel stitch, transport layer) and a launch on file.  Host-only: nothing here touches the device.
#include "same_harvest.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <new>
#include <string>
#include <utility>
#ifdef SAME_HOST_PROF
#include <x86intrin.h>
#endif

namespace same {

namespace {
thread_local std::string g_last_error;
}  // namespace

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}
const char *last_error() { return g_last_error.c_str(); }

// SAME_HOST_PROF (measurement builds: SAME_EXTRA_DEFS=SAME_HOST_PROF=1): time-stamp-counter totals of the replay's parts,
// printed by same_debug_harvest_replay (one thread); nothing in the product build
#ifdef SAME_HOST_PROF
static uint64_t g_hp[8];
static const char *const g_hp_name[8] = {"range sort", "poll synthesis", "queue record + payload", "transport: burst", "transport: other", "after_event", "stitch scan", "-"};
struct HpScope { int k; uint64_t t0; explicit HpScope(int k_) : k(k_), t0(__rdtsc()) {} ~HpScope() { g_hp[k] += __rdtsc() - t0; } };
#define HP(k) HpScope hp_scope_##k(k)
#else
#define HP(k) do {} while (0)
#endif

// a queue record as the event the ABI hands out
static void materialise(const QEvent &q, const uint8_t *arena, size_t arena_base, same_rx_event *ev)
{
    std::memset(ev, 0, sizeof(*ev));
    ev->kind = q.kind; ev->channel = q.channel; ev->sample_counter = q.sample_counter; ev->symbol_count = q.symbol_count;
    ev->len = q.len; ev->aux = q.aux; ev->aux2 = q.aux2;
    if (q.n_bytes) std::memcpy(ev->bytes, arena + (q.payload - arena_base), q.n_bytes);
}

// ---- EventLog ------------------------------------------------------------------------------------------------------

// The view same_batch_peek_events handed out is tens of MB for a large queue and is not kept for the handle's life -- but the
// header promises it stays readable across same_batch_drop_events, so a drop that empties the queue only marks it; the next
// call that ends the view's life anyway (poll, peek, a harvest, reset) lets the memory go.
void EventLog::release_stale_view()
{
    if (!peeked_release) return;
    peeked_release = false;
    if (!peeked_valid) std::vector<same_rx_event>().swap(peeked);
}
// the queue is empty: nothing refers to the arena any more
void EventLog::queue_emptied(bool view_may_be_read)
{
    queue.clear(); queue_head = 0; arena.clear();
    peeked_valid = false; peeked_head = 0;
    if (view_may_be_read) peeked_release = true;
    else { peeked_release = false; std::vector<same_rx_event>().swap(peeked); }
}

void EventLog::clear()
{
    queue.clear(); queue_head = 0;
    arena.clear();
    peeked_valid = false; peeked_release = false; peeked_head = 0;
    std::vector<same_rx_event>().swap(peeked);
    burst_seq.clear(); burst_seq_head = 0;
}

// A consumer that always polls less than is pending never drains the queue: reclaim the
// polled prefix once it is at least as large as what is still waiting (amortised O(1) per event).
int EventLog::begin_append(size_t n_records, size_t n_bytes, QEvent **dst, uint8_t **bdst, size_t *byte0)
{
    peeked_valid = false;                 // (the queue is about to move and grow: a materialised view of it is stale)
    release_stale_view();
    if (queue_head && queue_head >= queue.size() - queue_head) {
        queue_head = queue.compact(queue_head);
        // ... and the payload bytes in front of the first record that is still queued
        size_t keep_from = arena.base + arena.size();
        for (size_t i = 0; i < queue.size(); ++i)
            if (queue.data()[i].n_bytes) { keep_from = (size_t)queue.data()[i].payload; break; }
        arena.compact(keep_from - arena.base);
        ++n_queue_reclaims;
    }
    *dst = queue.grow(n_records);
    if (n_records && !*dst) return fail(SAME_ENOMEM, "event queue");
    *bdst = arena.grow(n_bytes);
    if (n_bytes && !*bdst) return fail(SAME_ENOMEM, "event payloads");
    *byte0 = arena.base + (arena.size() - n_bytes);
    return SAME_OK;
}

int EventLog::append_parts(WorkerPool &workers, std::vector<HarvestPart> &parts)
{
    using Part = HarvestPart;
    size_t total = 0, total_bytes = 0;
    for (const Part &p : parts) { total += p.out.size(); total_bytes += p.bytes.size(); }
    QEvent *dst = nullptr;
    uint8_t *bdst = nullptr;
    size_t byte0 = 0;
    if (const int rc = begin_append(total, total_bytes, &dst, &bdst, &byte0)) return rc;
    {
        // every thread's slice lands at its prefix offset; the copies run side by side
        size_t at = 0, bat = 0;
        if (burst_seq_head > 4096 && burst_seq_head * 2 > burst_seq.size()) {
            burst_seq.erase(burst_seq.begin(), burst_seq.begin() + (std::ptrdiff_t)burst_seq_head);
            burst_seq_head = 0;
            ++n_index_trims;
        }
        const size_t seq0 = queue.base + (queue.size() - total);
        struct Job { QEvent *q; uint8_t *b; Part *p; size_t byte_off; };
        std::vector<Job> jobs;
        for (size_t t = 0; t < parts.size(); ++t) {
            Part &p = parts[t];
            if (p.out.empty()) continue;
            for (uint32_t i : p.bursts) burst_seq.push_back(seq0 + at + i);
            jobs.push_back(Job{dst + at, bdst + bat, &p, byte0 + bat});
            at += p.out.size(); bat += p.bytes.size();
        }
        workers.run(jobs.size(), [&](size_t j) {
            const Job &job = jobs[j];
            for (QEvent &q : job.p->out) q.payload += job.byte_off;            // part-relative -> absolute
            std::memcpy(job.q, job.p->out.data(), job.p->out.size() * sizeof(QEvent));
            if (!job.p->bytes.empty()) std::memcpy(job.b, job.p->bytes.data(), job.p->bytes.size());
        });
    }
    return SAME_OK;
}

// n queue records as the events the ABI hands out, side by side when there are many
void EventLog::materialise_range(WorkerPool &workers, const QEvent *q, size_t n, same_rx_event *out)
{
    const uint8_t *arena_at = arena.data();
    const size_t abase = arena.base;
    if (n >= 4096) {
        const unsigned hw = std::thread::hardware_concurrency();
        const size_t n_threads = std::min<size_t>({8u, hw ? hw : 1u});
        workers.run(n_threads, [&](size_t t) {
            for (size_t i = n * t / n_threads; i < n * (t + 1) / n_threads; ++i) materialise(q[i], arena_at, abase, out + i);
        });
    } else {
        for (size_t i = 0; i < n; ++i) materialise(q[i], arena_at, abase, out + i);
    }
}

int EventLog::poll(WorkerPool &workers, same_rx_event *out, size_t cap, size_t *n_out, size_t *n_left)
{
    release_stale_view();
    const size_t avail = queue.size() - queue_head;
    const size_t n = std::min(cap, avail);
    materialise_range(workers, queue.data() + queue_head, n, out);
    queue_head += n;
    if (queue_head == queue.size()) queue_emptied();
    if (n_out) *n_out = n;
    if (n_left) *n_left = queue.size() - queue_head;
    return SAME_OK;
}

int EventLog::peek(WorkerPool &workers, const same_rx_event **events, size_t *n)
{
    // (the queue holds compact records: the view is made here, and stays valid as the header promises -- until the next
    // call on this handle other than same_batch_pending_events / same_batch_drop_events)
    release_stale_view();
    const size_t avail = queue.size() - queue_head;
    if (peeked_valid && peeked_head == queue_head && peeked.size() == avail) {     // (nothing was queued or dropped since)
        *n = avail; *events = avail ? peeked.data() : nullptr;
        return SAME_OK;
    }
    if (peeked_valid && peeked_head <= queue_head && queue_head - peeked_head <= peeked.size() &&
        peeked.size() - (queue_head - peeked_head) == avail) {
        // only drops since the last peek (the usual consumer: peek, keep a few, drop): the view moves up, nothing is rebuilt
        peeked.erase(peeked.begin(), peeked.begin() + (ptrdiff_t)(queue_head - peeked_head));
        peeked_head = queue_head;
        *n = avail; *events = avail ? peeked.data() : nullptr;
        return SAME_OK;
    }
    try { peeked.resize(avail); } catch (...) { return fail(SAME_ENOMEM, "event view"); }
    peeked_valid = true; peeked_head = queue_head;
    same_rx_event *out = peeked.data();
    materialise_range(workers, queue.data() + queue_head, avail, out);
    *n = avail;
    *events = avail ? out : nullptr;
    return SAME_OK;
}

int EventLog::drop(size_t n)
{
    if (n > queue.size() - queue_head) return fail(SAME_EINVAL, "more events than are queued");
    queue_head += n;
    if (queue_head == queue.size()) queue_emptied(/*view_may_be_read=*/true);
    return SAME_OK;
}

int EventLog::pack_bursts(WorkerPool &workers, uint32_t first_channel, uint8_t *out, size_t cap, size_t *n_records)
{
    static_assert(SAME_BURST_RECORD_BYTES == 16 + SAME_EVENT_MAX_BYTES, "record layout");
    // the queued bursts by the index the harvest keeps (no scan of the whole queue: bursts are a fifth of the events)
    const size_t first_seq = queue.base + queue_head;
    while (burst_seq_head < burst_seq.size() && burst_seq[burst_seq_head] < first_seq) ++burst_seq_head;
    const size_t n_b = burst_seq.size() - burst_seq_head;
    const size_t *seq = burst_seq.data() + burst_seq_head;
    const QEvent *q = queue.data();
    const size_t base = queue.base;
    const uint8_t *arena_at = arena.data();
    const size_t abase = arena.base;
    *n_records = n_b;
    if (!out || !cap) return SAME_OK;
    const size_t n_copy = std::min(n_b, cap);
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t n_threads = n_copy >= 8192 ? std::min<size_t>({8u, hw ? hw : 1u}) : 1u;
    auto copy_slice = [&](size_t t) {
        for (size_t i = n_copy * t / n_threads; i < n_copy * (t + 1) / n_threads; ++i) {
            const QEvent &e = q[seq[i] - base];
            uint8_t *r = out + i * SAME_BURST_RECORD_BYTES;
            const uint32_t ch = e.channel + first_channel, len = e.n_bytes;
            std::memcpy(r, &ch, 4); std::memcpy(r + 4, &e.sample_counter, 8); std::memcpy(r + 12, &len, 4);
            if (len) std::memcpy(r + 16, arena_at + ((size_t)e.payload - abase), len);
            std::memset(r + 16 + len, 0, SAME_EVENT_MAX_BYTES - len);
        }
    };
    workers.run(n_threads, copy_slice);
    return SAME_OK;
}

// ---- AudioLog ------------------------------------------------------------------------------------------------------

AudioChunk *AudioLog::grow(size_t n_chunks, size_t n_samples, float **samples_at, uint64_t *at)
{
    if (head && head >= queue.size() - head) {
        head = queue.compact(head);
        const uint64_t keep_from = queue.size() ? queue.data()[0].at : samples.base + samples.size();
        samples.compact((size_t)(keep_from - samples.base));
        ++n_reclaims;
    }
    AudioChunk *dst = queue.grow(n_chunks);
    if (n_chunks && !dst) return nullptr;
    float *sdst = samples.grow(n_samples);
    if (n_samples && !sdst) { queue.n -= n_chunks; return nullptr; }
    *samples_at = sdst;
    *at = samples.base + (samples.size() - n_samples);
    return dst;
}

int AudioLog::end_reset(const std::vector<uint32_t> &chans, uint64_t pos, const ResetLedger &resets)
{
    if (open.empty()) return SAME_OK;
    size_t n = 0;
    for (uint32_t c : chans) n += open[c];
    if (!n) return SAME_OK;
    float *sdst = nullptr;
    uint64_t at = 0;
    AudioChunk *dst = grow(n, 0, &sdst, &at);
    if (!dst) return fail(SAME_ENOMEM, "audio queue");
    for (uint32_t c : chans) {
        if (!open[c]) continue;
        *dst++ = AudioChunk{c, SAME_AUDIO_END_RESET, resets.rebase(c, pos), 0, at};
        open[c] = 0;
    }
    return SAME_OK;
}

int AudioLog::peek(const same_audio_chunk **chunks, size_t *n)
{
    const size_t avail = queue.size() - head;
    try { view.resize(avail); } catch (...) { return fail(SAME_ENOMEM, "audio view"); }
    const AudioChunk *q = queue.data() + head;
    for (size_t i = 0; i < avail; ++i) {
        same_audio_chunk &o = view[i];
        o.channel = q[i].channel; o.flags = q[i].flags; o.sample_counter = q[i].sample_counter; o.n_samples = q[i].n;
        o.samples = samples.data() + (size_t)(q[i].at - samples.base);
    }
    *n = avail;
    *chunks = avail ? view.data() : nullptr;
    return SAME_OK;
}

int AudioLog::drop(size_t n)
{
    if (n > queue.size() - head) return fail(SAME_EINVAL, "more chunks than are queued");
    head += n;       // (the memory is reclaimed by the next harvest that queues chunks: a view may still be read)
    return SAME_OK;
}

void AudioLog::clear()
{
    queue.clear(); head = 0; samples.clear();
    std::vector<same_audio_chunk>().swap(view);
    std::fill(open.begin(), open.end(), 0);
}

// ---- Replay --------------------------------------------------------------------------------------------------------

void Replay::init(uint32_t channels, uint32_t rate, bool host_transport)
{
    n_channels = channels; input_rate = rate;
    if (host_transport) { thot.resize(channels); tcold.resize(channels); }
    if (time_parallel) { sym_off.assign(channels, 0); synth.assign(channels, TickSynth{}); }
}

void Replay::reset()
{
    for (uint32_t c = 0; c < (uint32_t)thot.size(); ++c) tr(c).reset();
    for (auto &o : sym_off) o = 0;
    for (auto &t : synth) t.reset();
}

void Replay::reset_channel(uint32_t c, uint64_t pos)
{
    if (!thot.empty()) tr(c).reset();
    if (time_parallel) {
        sym_off[c] = 0;
        synth[c].reset();
        synth[c].a_t = pos;
    }
}

int Replay::replay(const HarvestLaunch &sl, const HarvestInput &in, uint32_t n_events, uint32_t n_bursts, std::vector<uint32_t> &rearm,
                   HarvestTimes &times)
{
    const bool dbg = debug;
    const DevEvent *evs = in.events;
    const uint8_t *bursts = in.bursts;
    const uint32_t n_ch = n_channels;
    const uint32_t n_bins = sl.chunked ? sl.geom.n_chunks * n_ch : n_ch;     // state columns of the launch
    // Per column the device emits in time order (a lane takes its log slots one after the other); across lanes the
    // atomic cursor interleaves.  The device has counted the events per column and moved the records into column
    // ranges (launch_event_sort: `evs` is that ordered copy, a record's `channel` holding its index in the log); inside
    // a range they stand in the order the scatter's atomics landed, and the replay threads sort each range (a handful
    // of records) back into log order = time order before they walk it.
    // (slots a wavefront reserved but did not use carry kDevEventNone and were skipped there)
    std::vector<uint32_t> first(in.first, in.first + n_bins + 1u);
    DevEvent *evs_mut = in.events;
    const uint32_t n_real = first[n_bins];
    if (n_real > n_events) return fail(SAME_EHIP, "internal: event sort counted %u of %u events", n_real, n_events);
    // (what follows indexes the ordered copy directly)
    struct Identity { uint32_t operator[](uint32_t i) const { return i; } } order;
    if (dbg && sl.chunked && sl.per_channel) {
        // how the per-channel boundaries came out: chunk lengths (own range + warm-up) and run-ons, in samples
        const ChunkGeom &g = sl.geom;
        const uint32_t *own = in.geom, *rows = in.geom + n_bins;
        double len_sum = 0, run_sum = 0; uint64_t len_max = 0, run_max = 0, n_len = 0, n_run = 0, n_inf = 0, n_late = 0;
        uint32_t worst_c = 0;
        for (uint32_t k = 0; k + 1u < g.n_chunks; ++k)
            for (uint32_t c = 0; c < n_ch; ++c) {
                const uint64_t end = own[(size_t)(k + 1u) * n_ch + c], len = end - rows[(size_t)k * n_ch + c];
                len_sum += (double)len; if (len > len_max) { len_max = len; worst_c = c; } ++n_len;
                const uint64_t h = in.handover[(size_t)k * n_ch + c];
                if (h == kNoHandover) { ++n_inf; continue; }
                const uint64_t run = h - g.counter0 > end ? h - g.counter0 - end : 0;
                run_sum += (double)run; run_max = std::max(run_max, run); ++n_run; n_late += run > 2u * g.block_len;
            }
        std::fprintf(stderr, "[same] longest piece on channel %u, its cuts:", worst_c);
        for (uint32_t k = 0; k < g.n_chunks; ++k) std::fprintf(stderr, " %u", own[(size_t)k * n_ch + worst_c]);
        std::fprintf(stderr, "\n");
        std::fprintf(stderr, "[same] per-channel chunks: length mean %.0f max %llu samples; run-on mean %.0f max %llu, %llu of %llu columns ran on "
                             "more than two blocks, %llu never handed over\n", len_sum / std::max<uint64_t>(n_len, 1), (unsigned long long)len_max,
                     run_sum / std::max<uint64_t>(n_run, 1), (unsigned long long)run_max, (unsigned long long)n_late, (unsigned long long)n_run,
                     (unsigned long long)n_inf);
    }
    // events per real channel, cumulative (a chunked launch spreads a channel over n_chunks columns)
    std::vector<uint32_t> chan_first;
    if (sl.chunked) {
        chan_first.assign(n_ch + 1u, 0u);
        for (uint32_t k = 0; k < sl.geom.n_chunks; ++k)
            for (uint32_t c = 0; c < n_ch; ++c) chan_first[c + 1u] += first[k * n_ch + c + 1u] - first[k * n_ch + c];
        for (uint32_t c = 0; c < n_ch; ++c) chan_first[c + 1u] += chan_first[c];
    }
    const std::vector<uint32_t> &cfirst = sl.chunked ? chan_first : first;
    const bool link_only = this->link_only;      // (locals, as the flags below: the replay's loops read them per event)
    const bool tp = time_parallel;
    times.sorted = std::chrono::steady_clock::now();

    // Channels are independent (one Transport each), so contiguous channel ranges are replayed
    // on separate host threads; each produces its slice of the output queue, in order.
    using Part = HarvestPart;
    const double sps = (double)input_rate / 520.83;
    const uint64_t interburst = max_interburst_symbols(), history = max_history_duration();
    // one device event -> the link event of channel c (+ the transport event it causes).  `off`: what
    // the time-parallel mode adds to the device's symbol count (0 otherwise).
    // (transport events arrive as same_rx_event from the transport layer: kept as a record + payload)
    // (the stitch and the transport layer work on the device's counters, from the batch's first sample; a queue record counts
    // from its channel's last reset: same_batch_reset_channels)
    const bool msgs_only = messages_only;
    auto push_transport = [&](Part &part, const same_rx_event &tev, uint32_t c) {
        if (msgs_only && tev.kind != SAME_TRANSPORT_MSG_START && tev.kind != SAME_TRANSPORT_MSG_END) return;
        QEvent q{};
        q.kind = tev.kind; q.channel = c; q.sample_counter = resets.rebase(c, tev.sample_counter); q.symbol_count = tev.symbol_count;
        q.len = tev.len; q.aux = tev.aux; q.aux2 = tev.aux2;
        q.n_bytes = std::min<uint32_t>(tev.len, SAME_EVENT_MAX_BYTES);
        if (tev.kind != SAME_TRANSPORT_MSG_START) q.n_bytes = 0;       // (only a header carries bytes)
        q.payload = part.bytes.size();
        if (q.n_bytes) part.bytes.insert(part.bytes.end(), tev.bytes, tev.bytes + q.n_bytes);
        part.out.push_back(q);
    };
    auto feed = [&](Part &part, same_rx_event &tev, const DevEvent &d, uint32_t c, int64_t off) {
        const uint64_t sym = (uint64_t)((int64_t)d.symbol_count + off);
        auto poll = [&](uint64_t psym, uint64_t pt) {
            if (tr(c).on_link_event(kDevTick, pt, psym, nullptr, 0, input_rate, &tev)) push_transport(part, tev, c);
        };
        if (tp && !link_only) {
            HP(1);
            synth[c].run_until(sym, d.sample_counter, sps, tr(c).force_eom_at(), poll);
        }
        QEvent q{};
        const uint8_t *payload = nullptr;
        {
        HP(2);
        q.kind = d.kind; q.channel = c; q.sample_counter = resets.rebase(c, d.sample_counter); q.symbol_count = sym;
        if (d.kind == SAME_LINK_BURST) {
            q.len = d.burst_len;
            if (d.burst_slot < n_bursts) {
                q.n_bytes = std::min<uint32_t>(d.burst_len, SAME_EVENT_MAX_BYTES);
                payload = bursts + (size_t)d.burst_slot * kBurstCap;
                q.payload = part.bytes.size();
                if (!msgs_only) part.bytes.insert(part.bytes.end(), payload, payload + q.n_bytes);
            } else {
                q.len = 0;     // pool overflow: the burst bytes were lost (SAME_EOVERFLOW is reported)
            }
            if (!msgs_only) part.bursts.push_back((uint32_t)part.out.size());
        }
        if (d.kind <= SAME_LINK_BURST && !msgs_only) part.out.push_back(q);
        }
        if (!link_only) {
#ifdef SAME_HOST_PROF
            HpScope hp_tr(d.kind == SAME_LINK_BURST ? 3 : 4);
#endif
            if (tr(c).on_link_event(d.kind, d.sample_counter, sym, payload, q.n_bytes, input_rate, &tev)) push_transport(part, tev, c);
            if (!tp && tr(c).force_eom_dirty()) part.rearm.push_back(c);
        }
        { HP(5); if (tp && d.kind <= SAME_LINK_BURST) synth[c].after_event(d.kind, sym, d.sample_counter, interburst, history); }
    };
    // Time-parallel launch: the events of channel c, stitched from its chunks.  Chunk `cur` is kept up to
    // its hand-over instant h (the end of the first block at or after its nominal end in which the
    // device saw it idle), then the chunk that owns h takes over -- from h if it is idle there too,
    // otherwise from its own next NoCarrier on (it was still busy with the tail of a burst it joined in
    // the middle, or with a duplicate of the burst the previous chunk has just delivered).
    auto stitch = [&](Part &part, same_rx_event &ev, uint32_t c) {
        const ChunkGeom &g = sl.geom;
        const uint64_t *hand = in.handover;
        // per-channel boundaries: own_start[k][c] and row0[k][c] as the device planned them
        const uint32_t *own = sl.per_channel ? in.geom : nullptr, *rows = sl.per_channel ? in.geom + n_bins : nullptr;
        auto owner_of = [&](uint64_t h) -> uint32_t {
            if (!own) return g.owner_of(h);
            uint32_t k = 0;
            while (k + 1u < g.n_chunks && g.counter0 + own[(size_t)(k + 1u) * n_ch + c] <= h) ++k;
            return k;
        };
        TickSynth &ts = synth[c];
        int64_t off = sym_off[c];
        uint32_t cur = 0;
        uint64_t keep_after = 0;
        for (;;) {
            const uint32_t col = cur * n_ch + c;
            const uint64_t h = hand[col];
            const uint64_t upto = std::min(h, sl.end_blocks);
            bool rebased = cur == 0;
            for (uint32_t i = first[col]; i < first[col + 1u]; ++i) {
                const DevEvent &d = evs[order[i]];
                if (d.sample_counter <= keep_after) continue;
                if (d.sample_counter > upto) break;
                if (!rebased) {
                    // continue the channel's symbol clock: the last reported event plus the nominal symbol rate
                    const int64_t est = (int64_t)ts.a_sym + (int64_t)((double)(d.sample_counter - ts.a_t) / sps + 0.5);
                    off = est - (int64_t)d.symbol_count;
                    rebased = true;
                }
                feed(part, ev, d, c, off);
            }
            if (!rebased) {
                // nothing reported from this chunk: its counter started at 0 at its first row
                const uint64_t row0 = rows ? g.counter0 + rows[col] : g.counter0 + (uint64_t)cur * g.stride_blocks * g.block_len;
                const int64_t est_end = (int64_t)ts.a_sym + (int64_t)((double)(sl.end_blocks - ts.a_t) / sps + 0.5);
                off = est_end - (int64_t)((double)(sl.end_blocks - row0) / sps + 0.5);
            }
            if (h == kNoHandover) break;
            const uint32_t nxt = owner_of(h);
            if (nxt <= cur) break;
            // the next chunk's link state at h, and where it is first idle from there on
            const uint32_t ncol = nxt * n_ch + c;
            uint32_t st = 0, j = first[ncol];
            for (; j < first[ncol + 1u] && evs[order[j]].sample_counter <= h; ++j)
                if (evs[order[j]].kind <= SAME_LINK_BURST) st = evs[order[j]].kind;
            keep_after = h;
            if (st == SAME_LINK_READING || st == SAME_LINK_BURST) {
                // busy with a burst the previous chunk has already delivered (or with the garbage a chunk that
                // joined in the middle of one makes of it): its events count from its next NoCarrier on
                for (; j < first[ncol + 1u]; ++j)
                    if (evs[order[j]].kind == SAME_LINK_NO_CARRIER) { keep_after = evs[order[j]].sample_counter; break; }
            } else if (st == SAME_LINK_SEARCHING && ts.link == SAME_LINK_NO_CARRIER) {
                // it has byte sync where the previous chunk has none yet (the two acquire a preamble some
                // symbols apart): what follows -- Reading, Burst -- is real, so the channel is Searching from here
                DevEvent inj{};
                inj.channel = ncol; inj.kind = SAME_LINK_SEARCHING; inj.sample_counter = h;
                inj.symbol_count = ts.a_sym + (uint64_t)((double)(h > ts.a_t ? h - ts.a_t : 0) / sps + 0.5);
                inj.burst_slot = 0xffffffffu;
                feed(part, ev, inj, c, 0);
            }
            cur = nxt;
        }
        // the remainder of the call (less than a block), demodulated on the channel's real state afterwards,
        // logs under column c like chunk 0
        for (uint32_t i = first[c]; i < first[c + 1u]; ++i)
            if (evs[order[i]].sample_counter > sl.end_blocks) feed(part, ev, evs[order[i]], c, off);
        sym_off[c] = off;
    };
    auto run_range = [&](uint32_t c0, uint32_t c1, Part &part) {
        part.out.clear(); part.bytes.clear(); part.rearm.clear(); part.bursts.clear();
        part.out.reserve((size_t)(cfirst[c1] - cfirst[c0]) * 3 / 2 + 4);
        same_rx_event ev;                                  // (scratch for what the transport layer returns)
        std::memset(&ev, 0, sizeof(ev));
        for (uint32_t c = c0; c < c1; ++c) {
            // (the next channel's transport state: its hot line is in the cache as a rule -- 2 MB for 32 768 channels -- the burst
            // history and message texts are not: all of them when a burst is on its way there)
            if (!link_only && c + 1u < c1) {
                __builtin_prefetch(&thot[c + 1u]);
                if (!sl.chunked) {
                    bool burst = false;
                    for (uint32_t k = first[c + 1u]; k < first[c + 2u]; ++k) burst |= evs[k].kind == SAME_LINK_BURST;
                    const char *nx = reinterpret_cast<const char *>(&tcold[c + 1u]);
                    if (burst) for (size_t o = 0; o < sizeof(TransportCold); o += 64) __builtin_prefetch(nx + o);
                }
            }
            // this channel's column ranges back into log order (see above)
            { HP(0);
            for (uint32_t col = c; col < n_bins; col += n_ch)
                if (first[col + 1u] - first[col] > 1u)
                    std::sort(evs_mut + first[col], evs_mut + first[col + 1u],
                              [](const DevEvent &a, const DevEvent &b) { return a.channel < b.channel; });
            }
            if (sl.chunked) stitch(part, ev, c);
            else
                for (uint32_t k = first[c]; k < first[c + 1u]; ++k)
                    feed(part, ev, evs[order[k]], c, tp ? sym_off[c] : 0);
            if (tp && !link_only) {
                // polls due before the end of this launch (the next launch's events start after it)
                TickSynth &ts = synth[c];
                if (ts.link == SAME_LINK_NO_CARRIER && sl.end_counter > ts.a_t) {
                    const uint64_t sym_end = ts.a_sym + (uint64_t)((double)(sl.end_counter - ts.a_t) / sps);
                    auto poll = [&](uint64_t psym, uint64_t pt) {
                        if (tr(c).on_link_event(kDevTick, pt, psym, nullptr, 0, input_rate, &ev)) push_transport(part, ev, c);
                    };
                    ts.run_until(sym_end + 1u, sl.end_counter + 1u, sps, tr(c).force_eom_at(), poll);
                }
            }
        }
    };
    uint32_t n_threads = 1;
    if (n_real >= 16384u && n_ch >= 64u) {
        const unsigned hw = std::thread::hardware_concurrency();
        // up to 32 replay threads, at most an eighth of the host's hardware threads (eight ranks share a node)
        n_threads = std::min<uint32_t>({32u, std::max(16u, hw / 8u), hw ? hw : 1u, n_ch / 32u});
        // (Measured against the container's cgroup CPU quota in round 5 -- the GPU boxes give 16 CPUs of 256 visible: capping the
        // pool at the quota made the headline step host-bound (replay 1.3-1.6 ms on 16 threads, 2.17 ms per step) where 32 threads
        // finish it in 0.8 ms and 2.09 ms per step; a burst of 32 threads for under a millisecond per 2 ms step stays inside a
        // 16-CPU quota on average and is not throttled.)
        if (host_threads > 0) n_threads = (uint32_t)host_threads;
    }
    if (parts.size() < n_threads) parts.resize(n_threads);
    for (Part &p : parts) { p.out.clear(); p.bytes.clear(); p.rearm.clear(); p.bursts.clear(); }
    if (n_threads == 1) {
        run_range(0, n_ch, parts[0]);
    } else {
        // split by event count, on channel boundaries
        std::vector<uint32_t> cut(n_threads + 1u, n_ch);
        cut[0] = 0;
        for (uint32_t t = 1; t < n_threads; ++t) {
            const uint32_t target = (uint32_t)((uint64_t)n_real * t / n_threads);
            cut[t] = (uint32_t)(std::lower_bound(cfirst.begin(), cfirst.end(), target) - cfirst.begin());
            cut[t] = std::min(std::max(cut[t], cut[t - 1u]), n_ch);
        }
        workers.run(n_threads, [&](size_t t) { run_range(cut[t], cut[t + 1u], parts[t]); });
    }
    times.replayed = std::chrono::steady_clock::now();
    times.n_threads = n_threads;
    if (const int rc = log.append_parts(workers, parts)) return rc;
    for (Part &p : parts) rearm.insert(rearm.end(), p.rearm.begin(), p.rearm.end());
    return SAME_OK;
}

int Replay::append_messages(const DevMessage *near, uint32_t n_near, const DevMessage *far, uint32_t n_far)
{
    const uint32_t n_msgs = n_near + n_far;
    auto rec = [&](uint32_t i) -> const DevMessage & { return i < n_near ? near[i] : far[i - n_near]; };
    std::vector<uint32_t> order(n_msgs);
    size_t n_bytes = 0;
    for (uint32_t i = 0; i < n_msgs; ++i) {
        order[i] = i;
        if (rec(i).kind == SAME_TRANSPORT_MSG_START) n_bytes += std::min<uint32_t>(rec(i).len, kDevMessageText);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const DevMessage &x = rec(a), &y = rec(b);
        return x.channel != y.channel ? x.channel < y.channel : x.seq < y.seq;
    });
    QEvent *dst = nullptr;
    uint8_t *bdst = nullptr;
    size_t at = 0;
    if (const int rc = log.begin_append(n_msgs, n_bytes, &dst, &bdst, &at)) return rc;
    for (uint32_t k = 0; k < n_msgs; ++k) {
        const DevMessage &d = rec(order[k]);
        QEvent q{};
        q.kind = d.kind; q.channel = d.channel; q.sample_counter = resets.rebase(d.channel, d.sample_counter);
        q.symbol_count = d.symbol_count; q.len = d.len; q.aux = d.aux; q.aux2 = d.aux2;
        if (d.kind == SAME_TRANSPORT_MSG_START && d.len) {
            q.n_bytes = std::min<uint32_t>(d.len, kDevMessageText);
            q.payload = at;
            std::memcpy(bdst, d.text, q.n_bytes);
            bdst += q.n_bytes; at += q.n_bytes;
        }
        dst[k] = q;
    }
    return SAME_OK;
}

// ---- a harvest on file ---------------------------------------------------------------------------------------------

int write_harvest_file(const char *path, HarvestFileHeader h, const HarvestInput &in)
{
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return fail(SAME_EINVAL, "SAME_RECORD_HARVEST: cannot write %s", path);
    h.magic = kHarvestMagic;
    const uint32_t n_bins = h.n_bins, n_events = h.n_events, n_bursts = h.n_bursts;
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1;
    ok = ok && std::fwrite(in.first, sizeof(uint32_t), (size_t)n_bins + 1, f) == (size_t)n_bins + 1;
    ok = ok && (!n_events || std::fwrite(in.events, sizeof(DevEvent), n_events, f) == n_events);
    ok = ok && (!n_bursts || std::fwrite(in.bursts, kBurstCap, n_bursts, f) == n_bursts);
    if (h.chunked) {
        ok = ok && std::fwrite(in.handover, sizeof(uint64_t), n_bins, f) == n_bins;
        if (h.per_channel) ok = ok && std::fwrite(in.geom, sizeof(uint32_t), (size_t)2 * n_bins, f) == (size_t)2 * n_bins;
    }
    std::fclose(f);
    return ok ? SAME_OK : fail(SAME_EINVAL, "SAME_RECORD_HARVEST: short write to %s", path);
}

int read_harvest_file(const char *path, HarvestRecord &rec)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return fail(SAME_EINVAL, "cannot read %s", path);
    HarvestFileHeader &h = rec.h;
    bool ok = std::fread(&h, sizeof(h), 1, f) == 1 && h.magic == kHarvestMagic && h.n_bins >= h.n_channels && h.n_channels > 0;
    std::vector<uint32_t> &first = rec.first, &geom = rec.geom;
    std::vector<DevEvent> &ev0 = rec.events;
    std::vector<uint8_t> &bursts = rec.bursts;
    std::vector<uint64_t> &hand0 = rec.handover;
    if (ok) {
        first.resize((size_t)h.n_bins + 1); ev0.resize(h.n_events); bursts.resize((size_t)h.n_bursts * kBurstCap);
        ok = std::fread(first.data(), sizeof(uint32_t), first.size(), f) == first.size();
        ok = ok && (!h.n_events || std::fread(ev0.data(), sizeof(DevEvent), h.n_events, f) == h.n_events);
        ok = ok && (!h.n_bursts || std::fread(bursts.data(), kBurstCap, h.n_bursts, f) == h.n_bursts);
        if (ok && h.chunked) {
            hand0.resize(h.n_bins);
            ok = std::fread(hand0.data(), sizeof(uint64_t), h.n_bins, f) == h.n_bins;
            if (ok && h.per_channel) { geom.resize((size_t)2 * h.n_bins); ok = std::fread(geom.data(), sizeof(uint32_t), geom.size(), f) == geom.size(); }
        }
    }
    std::fclose(f);
    if (ok) {
        // a record is data from a file: nothing in it is trusted before it has been checked against the sizes that were read
        ok = first[h.n_bins] <= h.n_events && h.n_bins % h.n_channels == 0;
        for (size_t i = 0; ok && i < (size_t)h.n_bins; ++i) ok = first[i] <= first[i + 1];
        for (size_t i = 0; ok && i < ev0.size(); ++i)
            ok = (ev0[i].burst_slot == 0xffffffffu || ev0[i].burst_slot < h.n_bursts) && (ev0[i].kind == kDevEventNone || ev0[i].kind <= 8u);
        if (ok && h.chunked) {
            ok = h.geom.n_chunks >= 1 && (uint64_t)h.geom.n_chunks * h.n_channels == h.n_bins && h.geom.block_len >= 1 && h.geom.stride_blocks >= 1;
            for (size_t i = 0; ok && h.per_channel && i < geom.size(); ++i) ok = geom[i] <= 0x7fffffffu;
        } else if (ok) {
            ok = h.n_bins == h.n_channels;
        }
    }
    if (!ok) return fail(SAME_EINVAL, "%s is not a (consistent) harvest record", path);
    return SAME_OK;
}

long replay_harvest_file(const char *path, int threads, int reps, double *ms_out, const HarvestSeen *each)
{
    if (!path || reps <= 0 || !ms_out) return -(long)fail(SAME_EINVAL, "null argument");
    HarvestRecord rec;
    if (const int rrc = read_harvest_file(path, rec)) return -(long)rrc;
    const HarvestFileHeader &h = rec.h;
    const std::vector<DevEvent> &ev0 = rec.events;
    const std::vector<uint64_t> &hand0 = rec.handover;
    ResetLedger resets;
    EventLog log;
    Replay rp(resets, log);
    rp.link_only = (h.flags & SAME_BATCH_LINK_ONLY) != 0;
    if (std::getenv("SAME_REPLAY_LINK_ONLY")) rp.link_only = true;      // (what the transport layer's share is)
    rp.time_parallel = h.tp_enabled != 0; rp.host_threads = threads;
    rp.init(h.n_channels, h.input_rate, !(h.flags & SAME_BATCH_LINK_ONLY));
    resets.init(h.n_channels);
    HarvestLaunch sl;
    std::vector<DevEvent> ev = ev0;
    std::vector<uint64_t> hand = hand0;
    const HarvestInput in{rec.first.data(), ev.data(), rec.bursts.data(), hand.data(), rec.geom.data()};
    sl.chunked = h.chunked != 0; sl.per_channel = h.per_channel != 0;
    const uint64_t span = h.end_counter - h.geom.counter0;        // (an ordinary launch: geom is zero, the span the end counter -- fine for a stride)
    const double sps = (double)h.input_rate / 520.83;
    const uint64_t span_sym = (uint64_t)((double)span / sps);
    long produced = 0;
    int rc = SAME_OK;
    for (int r = 0; r < reps && rc == SAME_OK; ++r) {
        const uint64_t dt = span * (uint64_t)r, ds = span_sym * (uint64_t)r;
        for (size_t i = 0; i < ev0.size(); ++i) { ev[i] = ev0[i]; ev[i].sample_counter += dt; if (!sl.chunked) ev[i].symbol_count += ds; }
        for (size_t i = 0; i < hand0.size(); ++i) hand[i] = hand0[i] == kNoHandover ? hand0[i] : hand0[i] + dt;
        sl.geom = h.geom; sl.geom.counter0 += dt;
        sl.end_blocks = h.end_blocks + dt; sl.end_counter = h.end_counter + dt;
        std::vector<uint32_t> rearm;
        HarvestTimes times;
        const auto t0 = std::chrono::steady_clock::now();
        rc = rp.replay(sl, in, h.n_events, h.n_bursts, rearm, times);
        ms_out[r] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        produced = (long)log.pending();
        if (each && rc == SAME_OK) (*each)(r, rp, log, rearm);
        // the consumer's side: everything polled
        size_t n_b = 0;
        log.drop(log.pending());
        log.pack_bursts(rp.workers, 0, nullptr, 0, &n_b);
    }
#ifdef SAME_HOST_PROF
    { uint64_t tot = 0; for (int k = 0; k < 7; ++k) tot += g_hp[k];
      for (int k = 0; k < 7; ++k) std::fprintf(stderr, "[same prof] %-24s %8.3f Mclk per harvest (%4.1f %% of the instrumented parts)\n", g_hp_name[k], (double)g_hp[k] / reps / 1e6, tot ? 100.0 * (double)g_hp[k] / (double)tot : 0.0); }
#endif
    return rc == SAME_OK ? produced : -(long)rc;
}

}  // namespace same

extern "C" long same_debug_harvest_replay(const char *path, int threads, int reps, double *ms_out)
{
    return same::replay_harvest_file(path, threads, reps, ms_out, nullptr);
}
