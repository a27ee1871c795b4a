// same_harvest.h -- the host half of a harvest: the compact event queue a batch hands its events out of (EventLog), the queue of
// alert-audio chunks (AudioLog), the replay that turns a launch's ordered log into queue records (Replay: ordering, the
// time-parallel stitch, the transport layer) and a launch on file (SAME_RECORD_HARVEST, same_debug_harvest_replay).
// same_batch.cpp waits, copies the launch's log into host buffers and calls in here with plain pointers.
// Host-only (no HIP): tests/helpers/harvest_main.cpp drives it under ASan + UBSan and under TSan without a device
// (tests/test_harvest_cpu.py).
#ifndef SAME_HARVEST_H
#define SAME_HARVEST_H

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/same_rx.h"
#include "same_device.h"
#include "same_resets.h"
#include "same_transport.h"

namespace same {

// The library's one error channel: the thread-local message behind same_last_error().  Returns `code`.
int fail(int code, const char *fmt, ...);
const char *last_error();

// ------------------------------------------------------------------------------------
// The host event queue.  A harvest of configs[1] brings ~110 000 link events per step; as 328-byte same_rx_event
// records that was 36 MB written twice per step (thread-local parts, then the queue) -- 2 ms of host time under a
// 2.7 ms launch.  The queue therefore holds 48-byte records, the burst / header bytes of the few events that carry any
// sit in a byte arena beside them, and a same_rx_event is only made when a consumer asks for one
// (same_batch_poll_events / _peek_events; same_batch_pack_bursts reads the records directly).
struct QEvent {
    uint32_t kind, channel;
    uint64_t sample_counter, symbol_count;
    uint32_t len, aux, aux2;
    uint32_t n_bytes;                // payload bytes kept (min(len, SAME_EVENT_MAX_BYTES)), 0 = none
    uint64_t payload;                // absolute offset of the payload in the arena
};
static_assert(sizeof(QEvent) == 48, "compact event record");
template <typename T>
struct PodQueue {                    // a plain growable array of PODs (no zero-fill on growth, appendable in slices)
    T *buf = nullptr;
    size_t n = 0, cap = 0;
    size_t base = 0;                 // how many elements have left the front since the handle was made: buf[i] is number base + i
    ~PodQueue() { std::free(buf); }
    PodQueue() = default;
    PodQueue(const PodQueue &) = delete;
    PodQueue &operator=(const PodQueue &) = delete;
    size_t size() const { return n; }
    T *data() { return buf; }
    const T *data() const { return buf; }
    void clear() { base += n; n = 0; }
    // drop the first `head` elements by moving the rest to the front; returns the new head (0)
    size_t compact(size_t head)
    {
        if (head == 0) return 0;
        if (head < n) std::memmove(buf, buf + head, (n - head) * sizeof(T));
        n -= head;
        base += head;
        return 0;
    }
    // room for `extra` more elements; returns where they go, or nullptr when out of memory
    T *grow(size_t extra)
    {
        if (n + extra > cap) {
            const size_t want = (n + extra) + (n + extra) / 2 + 64;
            void *p = std::realloc(buf, want * sizeof(T));
            if (!p) return nullptr;
            buf = static_cast<T *>(p);
            cap = want;
        }
        T *at = buf + n;
        n += extra;
        return at;
    }
};
using EventQueue = PodQueue<QEvent>;
// a queued chunk of alert audio (same_batch_set_audio_capture): its samples are [at, at + n) of the sample arena (absolute index)
struct AudioChunk {
    uint32_t channel, flags;
    uint64_t sample_counter, n;
    uint64_t at;
};
using ByteArena = PodQueue<uint8_t>;     // payload bytes: element number = absolute offset
struct HarvestPart {
    std::vector<QEvent> out;             // payload = offset into `bytes` until the part is appended to the queue
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> rearm;
    std::vector<uint32_t> bursts;        // indices into out
};

// A few parked worker threads per batch for the harvest (replay, queue copy, burst packing): starting and joining 60
// std::threads per launch costs more than the work some of them do, and eight ranks share one host.
class WorkerPool {
public:
    ~WorkerPool()
    {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; }
        cv_.notify_all();
        for (std::thread &t : threads_) t.join();
    }
    // fn(0) .. fn(n - 1), the caller taking part; returns when all are done
    void run(size_t n, const std::function<void(size_t)> &fn)
    {
        if (n <= 1) { if (n) fn(0); return; }
        while (threads_.size() + 1 < n) threads_.emplace_back([this] { loop(); });
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn; next_ = 0; count_ = n; pending_ = n; ++generation_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void work()
    {
        for (;;) {
            size_t i;
            const std::function<void(size_t)> *fn;
            {
                std::lock_guard<std::mutex> g(mu_);
                if (!fn_ || next_ >= count_) return;
                i = next_++; fn = fn_;
            }
            (*fn)(i);
            std::lock_guard<std::mutex> g(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
            }
            work();
        }
    }
    std::vector<std::thread> threads_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)> *fn_ = nullptr;
    size_t next_ = 0, count_ = 0, pending_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};

// The ordered host-side event queue of a batch and the view same_batch_peek_events hands out.  The calls that copy many
// records take the batch's worker pool.
class EventLog {
public:
    // events already brought back to the host
    size_t pending() const { return queue.size() - queue_head; }
    int poll(WorkerPool &workers, same_rx_event *out, size_t cap, size_t *n_out, size_t *n_left);
    int peek(WorkerPool &workers, const same_rx_event **events, size_t *n);
    int drop(size_t n);
    int pack_bursts(WorkerPool &workers, uint32_t first_channel, uint8_t *out, size_t cap, size_t *n_records);
    // Before a harvest appends to the queue: room for n_records records at *dst and n_bytes payload bytes at *bdst, whose first
    // has the absolute arena offset *byte0
    int begin_append(size_t n_records, size_t n_bytes, QEvent **dst, uint8_t **bdst, size_t *byte0);
    // the replay threads' slices, in order, with their bursts into the burst index
    int append_parts(WorkerPool &workers, std::vector<HarvestPart> &parts);
    void clear();                       // event_queue.clear() receiver.rs:194
    // the queued records, oldest first, and a record's payload bytes (until the next call that is not const)
    const QEvent *records() const { return queue.data() + queue_head; }
    const uint8_t *payload_of(const QEvent &q) const { return arena.data() + ((size_t)q.payload - arena.base); }
    // how often the polled prefix of the queue / the consumed prefix of the burst index has been reclaimed
    uint64_t n_queue_reclaims = 0, n_index_trims = 0;

private:
    void materialise_range(WorkerPool &workers, const QEvent *q, size_t n, same_rx_event *out);
    void release_stale_view();
    void queue_emptied(bool view_may_be_read = false);
    EventQueue queue;                   // events not yet polled: [queue_head, size)
    size_t queue_head = 0;
    ByteArena arena;                    // their payload bytes
    std::vector<same_rx_event> peeked;  // same_batch_peek_events: the queued events, materialised (328 bytes each) ...
    bool peeked_valid = false;          // ... and whether it still mirrors queue[peeked_head ..) (a harvest appends: invalid)
    bool peeked_release = false;        // the queue ran empty under same_batch_drop_events: the caller may still be reading the view; freed by the next call that ends its life
    size_t peeked_head = 0;
    std::vector<size_t> burst_seq;      // event numbers (EventQueue::base + index) of the queued SAME_LINK_BURST events, ascending
    size_t burst_seq_head = 0;          // entries before this one have been polled or dropped
};

// alert audio per message (same_batch_set_audio_capture): the queued chunks and their samples
class AudioLog {
public:
    // per channel: a capture is open as far as the queued chunks go (END_RESET chunks); empty: capture is off
    std::vector<uint8_t> open;
    // Before chunks are appended to the audio queue: reclaim the dropped prefix once it is at least as large as what is still queued
    // (the queue and the sample arena move: a view of same_batch_peek_audio is stale by then anyway)
    AudioChunk *grow(size_t n_chunks, size_t n_samples, float **samples_at, uint64_t *at);
    // The channels' open captures end at a reset (same_batch_reset_channels) at batch position `pos`: an empty END_RESET chunk at the
    // counter the capture had reached.  Called once every chunk before `pos` is queued, before the channels' counter bases move.
    int end_reset(const std::vector<uint32_t> &chans, uint64_t pos, const ResetLedger &resets);
    // The spans of a launch that captured and the used part [0, used) of its sample pool, to the queue by (channel, emission
    // order) -- a lane lists its spans in counter order.  *n_samples_out: how many samples were queued.
    // (Span: same::cap::Span.  same_capture_dev.h is device code as well and wants the HIP runtime where this unit is built as
    // part of the library, so the type comes in with the caller)
    template <typename Span>
    int append_spans(const Span *sp, uint32_t n_spans, const float *pool, size_t used, const ResetLedger &resets, size_t *n_samples_out)
    {
        std::vector<uint32_t> order(n_spans);
        size_t n_samples = 0;
        for (uint32_t i = 0; i < n_spans; ++i) {
            order[i] = i;
            if (sp[i].n && sp[i].off + sp[i].n <= used) n_samples += sp[i].n;
        }
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sp[a].channel != sp[b].channel ? sp[a].channel < sp[b].channel : a < b; });
        float *sdst = nullptr;
        uint64_t at = 0;
        AudioChunk *dst = grow(n_spans, n_samples, &sdst, &at);
        if (!dst) return fail(SAME_ENOMEM, "audio queue");
        for (uint32_t k = 0; k < n_spans; ++k) {
            const Span &s = sp[order[k]];
            const uint32_t n = s.n && s.off + s.n <= used ? s.n : 0;
            uint32_t flags = s.flags;
            if (n < s.n) flags |= SAME_AUDIO_TRUNCATED;
            dst[k] = AudioChunk{s.channel, flags, resets.rebase(s.channel, s.counter), n, at};
            if (n) { std::memcpy(sdst, pool + s.off, (size_t)n * sizeof(float)); sdst += n; at += n; }
            if (flags & SAME_AUDIO_FIRST) open[s.channel] = 1;
            if (flags & (SAME_AUDIO_END_MESSAGE | SAME_AUDIO_END_FLUSH | SAME_AUDIO_END_RESET)) open[s.channel] = 0;
        }
        if (n_samples_out) *n_samples_out = n_samples;
        return SAME_OK;
    }
    int peek(const same_audio_chunk **chunks, size_t *n);
    int drop(size_t n);
    // the audio queue goes with the event queue, and every capture is closed
    void clear();
    uint64_t n_reclaims = 0;            // how often the dropped prefix has been reclaimed

private:
    PodQueue<AudioChunk> queue;              // chunks not yet dropped: [head, size)
    size_t head = 0;
    PodQueue<float> samples;                 // their samples (element number = absolute index)
    std::vector<same_audio_chunk> view;      // same_batch_peek_audio
};

struct HarvestTimes { std::chrono::steady_clock::time_point sorted, replayed; uint32_t n_threads = 1; };
// what the replay reads of a launch: the slot's landing buffers, or a recorded launch's (same_debug_harvest_replay)
struct HarvestInput {
    const uint32_t *first;           // [columns + 1] the columns' ranges of `events`
    DevEvent *events;                // each range is sorted in place
    const uint8_t *bursts;
    const uint64_t *handover;        // a time-parallel launch's
    const uint32_t *geom;            // ... with per-channel boundaries: own_start | row0
};
// ... and what it has to know about the launch itself
struct HarvestLaunch {
    bool chunked = false;            // time-parallel launch: geometry, the end of its last whole block
    bool per_channel = false;        // per-channel chunk boundaries (channel-major input)
    ChunkGeom geom{};
    uint64_t end_blocks = 0;
    uint64_t end_counter = 0;        // input sample counter after this launch
};

// The host state of a batch's channels and the replay of a launch over it
class Replay {
public:
    Replay(ResetLedger &resets_, EventLog &log_) : resets(resets_), log(log_) {}
    uint32_t n_channels = 0, input_rate = 0;
    bool link_only = false;             // SAME_BATCH_LINK_ONLY
    bool messages_only = false;         // SAME_BATCH_MESSAGES_ONLY: only MSG_START / MSG_END are queued
    bool time_parallel = false;         // SAME_BATCH_TIME_PARALLEL
    bool debug = false;                 // SAME_DEBUG: harvest statistics on stderr
    int host_threads = 0;               // SAME_HOST_THREADS: harvest threads (0 = choose)
    std::vector<HarvestPart> parts;     // per host thread, kept between harvests for their capacity
    WorkerPool workers;
    // transport layer, one assembler per channel (unless SAME_BATCH_LINK_ONLY)
    // (two arrays: one cache line per channel that every poll touches, and the burst bytes / message texts: same_transport.h)
    std::vector<TransportHot> thot;
    std::vector<TransportCold> tcold;
    TransportRef tr(uint32_t c) { return TransportRef(thot[c], tcold[c]); }
    // time-parallel mode
    std::vector<int64_t> sym_off;        // per channel: reported symbol count - the device's
    std::vector<TickSynth> synth;

    // the per-channel state of a new batch (host_transport: the transport layer runs here, not on the device)
    void init(uint32_t channels, uint32_t rate, bool host_transport);
    // the whole batch was reset (same_batch_reset)
    void reset();
    // The host half of a reset of channel c at stream position `pos` (same_batch_reset_channels): the transport layer goes Idle and
    // forgets its bursts, pending message and forced-EOM instant (receiver.rs:195-196); the time-parallel symbol clock restarts at
    // `pos` (the device's symbol counter of the channel restarts there too)
    void reset_channel(uint32_t c, uint64_t pos);
    // The host half of a harvest: the launch's ordered event log, burst pool, hand-over instants and chunk geometry are in
    // host buffers; order each column's records, replay the channels (stitch + transport layer) on the worker threads and
    // append to the queue.  Touches no device: same_debug_harvest_replay runs it on a recorded launch without one.
    int replay(const HarvestLaunch &L, const HarvestInput &in, uint32_t n_events, uint32_t n_bursts, std::vector<uint32_t> &rearm,
               HarvestTimes &times);
    // The message log of a launch that ran the transport layer on the device (SAME_BATCH_MESSAGES_ONLY), its first n_near
    // records at `near`, the rest at `far`.  The log's order across lanes is that of their atomics; the queue
    // takes it by channel and, per channel, in the order the lane logged it (= iter_events() filtered to messages).
    int append_messages(const DevMessage *near, uint32_t n_near, const DevMessage *far, uint32_t n_far);

private:
    ResetLedger &resets;
    EventLog &log;
};

// ---- a harvest on file (tools/host_step_probe.py --ranks N: the host half of a step without a device) ----------------
// SAME_RECORD_HARVEST=<path>: the third harvest of a batch writes what the host half reads -- the ordered log, the columns'
// offsets, the burst pool, hand-over instants and chunk geometry -- to <path>.
struct HarvestFileHeader {
    uint64_t magic;                  // "SAMEHRV1"
    uint32_t n_channels, n_bins, n_events, n_bursts, chunked, per_channel, flags, input_rate, tp_enabled, pad;
    ChunkGeom geom;
    uint64_t end_blocks, end_counter;
};
constexpr uint64_t kHarvestMagic = 0x3156524845'4d4153ull;
// (h.magic is set here; the arrays have the sizes the header states: n_bins + 1 offsets, n_events, n_bursts, and for a chunked
// launch n_bins hand-overs and, with per-channel boundaries, 2 n_bins geometry words)
int write_harvest_file(const char *path, HarvestFileHeader h, const HarvestInput &in);
// a record read back, every index in it checked against the sizes that were read
struct HarvestRecord {
    HarvestFileHeader h{};
    std::vector<uint32_t> first, geom;
    std::vector<DevEvent> events;
    std::vector<uint8_t> bursts;
    std::vector<uint64_t> handover;
};
int read_harvest_file(const char *path, HarvestRecord &rec);
// same_debug_harvest_replay (below); `each`, if given, sees every repetition's output before the consumer's side drops it
using HarvestSeen = std::function<void(int rep, const Replay &, const EventLog &, const std::vector<uint32_t> &rearm)>;
long replay_harvest_file(const char *path, int threads, int reps, double *ms_out, const HarvestSeen *each);

}  // namespace same

// The host half of a step on a recorded launch, `reps` times on `threads` harvest threads, without a device: wall time of
// each repetition in ms_out[reps] (the record's counters are moved on by the launch's length every time, so the transport
// layer sees a stream that continues).  Returns the number of queue records one repetition produced, or a negative error.
extern "C" long same_debug_harvest_replay(const char *path, int threads, int reps, double *ms_out);

#endif  // SAME_HARVEST_H
