// trc_host.inc -- layer 1 of libturborc_hip.so: the reference prototypes on HOST pointers (included by trc_api.hip).
//
// A TurboRC-style caller hands over pageable host buffers and times the whole call, so this layer is a PCIe pipeline:
//   * the buffer is cut into slices (whole groups of 64 chunks); slice i+1 is on its way to the GPU while slice i is coded and
//     slice i-1 travels back: an H2D stream, a D2H stream and SEVERAL coder streams tied by events, both DMA directions busy at
//     once (PCIe Gen5 x16 measured on the MI355X box: 57 GB/s one way, 48 GB/s each way when both run);
//   * round 6: the chunk is chosen for the RATIO the caller sees (trc_auto_chunk_codec: the largest chunk whose one-wave time
//     still hides behind the call's PCIe time), and a launch of large chunks is a launch of few, long waves -- one slice leaves
//     most of the chip idle for the whole of a wave's time.  So the slices of a call are coded CONCURRENTLY: slice i runs on
//     coder stream i % nks with workspace i % nks and a payload region of its own, the host reads the slices' sizes in order,
//     well behind the launches (up to TRC_NKEV slices in flight), and only then queues their way back;
//   * a hipMemcpyAsync on pageable memory returns only when the copy is done (measured: two directions from one thread
//     = 28 GB/s each), so transfers go through pinned staging buffers, filled and emptied by a small pool of copy threads
//     (one thread moves 28 GB/s, four 110 GB/s); registering the caller's buffers instead costs 5.5 ms per 100 MB and a
//     registration must not outlive memory the caller may free;
//   * one context per DEVICE (the caller's current device at the time of the call), each with its own lock: calls on one
//     device serialise, calls on different devices do not;
//   * round 6: a call may be spread over SEVERAL devices (trc_set_devices / TRC_DEVICES): contiguous shards of whole chunk
//     groups, one context and one host thread per listed device, every shard the same pipeline writing its directory slice and
//     its payload straight to their places in the caller's `out` -- the container is byte-identical to the one-device one.
//     This is how the reference's single-threaded harness (turborc.c:420-579) reaches the other GPUs of a node at all.
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <string>
#include <thread>
#include <vector>
namespace {
// ---- copy threads: memcpy(dst, src, len) split over the pool, caller blocks until done --------------------------
class CopyPool {
public:
    // A pool belongs to ONE HostCtx: two per context -- one fills the staging buffers on the way in, one empties
    // them on the way out, both directions at once -- created with the context and used only under the context's lock, so
    // calls on different devices never meet in a pool (round 2 had two process-wide pools behind per-device locks: two
    // threads could both pass wait() and the second overwrite the first's job).  Never destroyed: the threads are detached
    // and wait on the condition variable for the life of the process (destroying a condition variable with waiters blocks
    // in glibc: a process would hang at exit).
    // start a copy on the pool's threads and return; wait() blocks until it is done (one copy in flight per pool).
    // Waiting for the previous job and installing the new one happen under ONE lock, so start() is safe on its own too.
    void start(void *dst, const void *src, size_t len)
    {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        if (len == 0) return;
        if (nthr_ == 0) { lk.unlock(); memcpy(dst, src, len); return; }
        dst_ = (uint8_t *)dst; src_ = (const uint8_t *)src; len_ = len; next_ = 0; strided_ = false; pending_ = nthr_; gen_++;
        lk.unlock();
        cv_.notify_all();
    }
    void wait()
    {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
    }
    // copy with the caller's help, blocking
    void copy(void *dst, const void *src, size_t len)
    {
        if (len < (1u << 20)) { wait(); memcpy(dst, src, len); return; }
        start(dst, src, len);
        work();
        wait();
    }
    // 2-D copies: `rows` rows of `width` bytes, `spitch` apart in src, `dpitch` apart in dst (the k-th part of every chunk of a piece:
    // streamed decodes scatter rows from a staging slot to their chunks).  Returns at once (pool threads only; wait() or the next
    // start blocks until it is done).
    void start2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t rows)
    {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        if (!rows || !width) return;
        if (nthr_ == 0) { lk.unlock(); for (size_t r = 0; r < rows; r++) memcpy((uint8_t *)dst + r * dpitch, (const uint8_t *)src + r * spitch, width); return; }
        dst_ = (uint8_t *)dst; src_ = (const uint8_t *)src; width_ = width; spitch_ = spitch; dpitch_ = dpitch;
        rows_per_ = PIECE / width ? PIECE / width : 1;
        len_ = rows; next_ = 0; strided_ = true;                 // len_ / next_ count ROWS in this mode
        pending_ = nthr_; gen_++;
        lk.unlock();
        cv_.notify_all();
    }
    CopyPool()
    {
        const char *e = getenv("TRC_COPY_THREADS");
        nthr_ = e ? atoi(e) : 10;                                           // per pool (+ the calling thread in copy()); round 6: 6 -> 10 (2 x 64-core host, rccdfenc pageable 21.2 -> 25.5 GB/s, profiles/r06_host_pointer_pieces.txt)
        if (nthr_ < 0) nthr_ = 0;
        if (nthr_ > 15) nthr_ = 15;
        for (int i = 0; i < nthr_; i++) std::thread([this] { loop(); }).detach();
    }
    CopyPool(const CopyPool &) = delete;
private:
    static constexpr size_t PIECE = 1u << 19;
    void work()
    {
        for (;;) {
            size_t o, step;
            bool strided;
            { std::lock_guard<std::mutex> lk(mu_); if (next_ >= len_) return; strided = strided_; step = strided ? rows_per_ : PIECE; o = next_; next_ += step; }
            if (!strided) { memcpy(dst_ + o, src_ + o, len_ - o < PIECE ? len_ - o : PIECE); continue; }
            const size_t r1 = o + step < len_ ? o + step : len_;
            for (size_t r = o; r < r1; r++) memcpy(dst_ + r * dpitch_, src_ + r * spitch_, width_);
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return gen_ != seen; }); seen = gen_; }
            work();
            { std::lock_guard<std::mutex> lk(mu_); if (--pending_ == 0) done_.notify_all(); }
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_;
    uint8_t *dst_ = nullptr; const uint8_t *src_ = nullptr;
    size_t len_ = 0, next_ = 0, width_ = 0, spitch_ = 0, dpitch_ = 0, rows_per_ = 1;
    bool strided_ = false;
    int nthr_ = 0, pending_ = 0;
    uint64_t gen_ = 0;
};

#define TRC_NSLOT 3                                  // staging slots per direction
#define TRC_NKS_MAX 8                                // coder streams of a context at most (TRC_HOST_STREAMS, default 2)
#define TRC_NKEV 16                                  // slices whose coder kernels may be queued before the host has read their sizes
#define TRC_MAX_SLICES 2000                          // the totals area holds 4096
struct HostJob;
class OutWorker;
struct HostCtx {
    std::mutex mu;
    bool init = false;
    int dev = -1;
    int nks = 0;                                       // coder streams
    hipStream_t s_in = nullptr, s_out = nullptr, s_k[TRC_NKS_MAX] = {};
    uint8_t *d_in = nullptr;   size_t cap_in = 0;      // plain bytes (encode input / decode output) of the shard
    uint8_t *d_cont = nullptr; size_t cap_cont = 0;    // directory slice | payload regions of the shard
    uint8_t *d_base = nullptr; size_t cap_base = 0;    // the base of a planes call against one (trc_bplanes.inc)
    uint8_t *d_work[TRC_NKS_MAX] = {}; size_t cap_work[TRC_NKS_MAX] = {};   // one workspace per coder stream
    uint8_t *d_small = nullptr;                        // cdf (1 KiB) | totals (8 B x 4096 slices at 2048) | status
    // pageable caller buffers travel in PIECES (host_piece(): 8 MB) through three pinned slots per direction -- the unit of the
    // copies, independent of the slices, which are the unit of the kernels
    uint8_t *pin_in[TRC_NSLOT] = {}, *pin_out[TRC_NSLOT] = {}; size_t cap_pin = 0;
    uint64_t *pin_tot = nullptr;                       // pinned: per-slice totals
    uint32_t *pin_prog = nullptr;                      // pinned: 16 slices x 16 progress flags a streamed decode's kernels set, part by part
    uint32_t *pin_flags = nullptr;                     // pinned: the numbers 0 .. 64 (the values the arrival gate is set to, pass by pass)
    hipEvent_t ev_in[TRC_NSLOT] = {}, ev_out[TRC_NSLOT] = {}, ev_misc = nullptr;
    std::vector<hipEvent_t> ev_k, ev_h;                // per slice of a call: its coder kernels are done / its input has arrived (grown on demand, reused by later calls)
    size_t qin = 0;                                    // pieces pushed by the call in progress
    CopyPool *pool_in = nullptr, *pool_out = nullptr;  // this context's copy threads (staging in / unstaging out)
    OutWorker *out = nullptr;                          // this context's thread for the way back to pageable memory
};
// tuning aid: bytes of a chunk per pass of a striped encode / streamed decode (multiple of 128; default: chunk / 8, at least 1 KB)
size_t host_part_env()
{
    static const size_t v = [] { const char *e = getenv("TRC_HOST_PART"); size_t x = e ? (size_t)strtoull(e, 0, 10) : 0; return x & ~(size_t)127; }();
    return v;
}
size_t host_piece()
{
    static const size_t v = [] { const char *e = getenv("TRC_HOST_PIECE"); size_t x = e ? (size_t)strtoull(e, 0, 10) : (size_t)8 << 20;
                                 return x < 65536 ? (size_t)65536 : x > ((size_t)256 << 20) ? (size_t)256 << 20 : x & ~(size_t)255; }();
    return v;
}
// The way back to PAGEABLE caller memory runs on a thread of its own (one per context, living as long as the process): the
// thread that stages the input never waits for a D2H copy, and both directions of the link stay busy whatever the coder does in
// between.  A job = `len` device bytes for host address `host`, to be fetched once `after` has happened (an event of a coder
// stream; null: it already has).  The worker moves a job in pieces through the three pin_out slots: piece q's D2H is queued
// BEFORE piece q-1 leaves its slot (the D2H engine never waits for the host), the out-pool's threads do the leaving.
void job_fail(HostJob *J, const char *msg);
bool job_failed(HostJob *J);
class OutWorker {
public:
    // parts != 0: a STREAMED job (round 6, decodes): the device bytes are `rows` chunks of `chunk` bytes whose part k -- bytes
    // [k part, (k + 1) part) of every chunk -- may be fetched as soon as the kernel has set flags[k] (page-locked host memory, polled
    // here); `direct`: host is page-locked (one 2-D copy per part straight into it), else through the staging slots and scattered
    struct Job { HostJob *J; const uint8_t *dev; uint8_t *host; size_t len; hipEvent_t after;
                 size_t parts = 0, part = 0, chunk = 0, rows = 0; volatile uint32_t *flags = nullptr; bool direct = false; };
    explicit OutWorker(HostCtx &ctx) : c_(ctx) { std::thread([this] { loop(); }).detach(); }
    void submit(const Job &j)
    {
        { std::lock_guard<std::mutex> lk(mu_); q_.push_back(j); idle_ = false; }
        cv_.notify_one();
    }
    // everything submitted has landed in the caller's memory (or has failed: the job's HostJob carries the message)
    void drain()
    {
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return idle_; });
    }
private:
    struct Pend { HostJob *J; uint8_t *dst; size_t len; int slot; bool live; size_t rows = 0, width = 0, dpitch = 0; };
    bool fetch(Pend &p)
    {
        if (!p.live) return true;
        p.live = false;
        if (hipEventSynchronize(c_.ev_out[p.slot]) != hipSuccess) { job_fail(p.J, "host layer: waiting for a D2H copy failed"); return false; }
        if (p.rows) c_.pool_out->start2d(p.dst, p.dpitch, c_.pin_out[p.slot], p.width, p.width, p.rows);       // rows of a part back to their chunks
        else if (p.len < (1u << 18)) { c_.pool_out->wait(); memcpy(p.dst, c_.pin_out[p.slot], p.len); }
        else c_.pool_out->start(p.dst, c_.pin_out[p.slot], p.len);
        return true;
    }
    // a streamed job: wait for each part's flag, then fetch that part of every chunk
    void run_streamed(const Job &j, Pend &pend, size_t &q)
    {
        const size_t piece = host_piece();
        for (size_t k = 0; k < j.parts; k++) {
            const double t0 = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
            for (unsigned spins = 0; !j.flags[k]; spins++) {
                __builtin_ia32_pause();
                if ((spins & 0xfffu) == 0xfffu) {
                    if (job_failed(j.J)) return;
                    if (std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - t0 > 10.0) {
                        job_fail(j.J, "host layer: a decoder never reported a part of its output (progress flag timed out)"); return;
                    }
                }
            }
            const size_t w = j.chunk - k * j.part < j.part ? j.chunk - k * j.part : j.part;
            const uint8_t *src = j.dev + k * j.part;
            uint8_t *dst = j.host + k * j.part;
            if (j.direct) {
                if (hipMemcpy2DAsync(dst, j.chunk, src, j.chunk, w, j.rows, hipMemcpyDeviceToHost, c_.s_out) != hipSuccess) { job_fail(j.J, "host layer: queueing a 2-D D2H copy failed"); return; }
                continue;
            }
            const size_t rows_per = piece / w ? piece / w : 1;
            for (size_t r0 = 0; r0 < j.rows; r0 += rows_per, q++) {
                const size_t rows = j.rows - r0 < rows_per ? j.rows - r0 : rows_per;
                const int slot = (int)(q % TRC_NSLOT);
                if (hipMemcpy2DAsync(c_.pin_out[slot], w, src + r0 * j.chunk, j.chunk, w, rows, hipMemcpyDeviceToHost, c_.s_out) != hipSuccess ||
                    hipEventRecord(c_.ev_out[slot], c_.s_out) != hipSuccess) { job_fail(j.J, "host layer: queueing a 2-D D2H copy failed"); return; }
                if (!fetch(pend)) return;
                pend = { j.J, dst + r0 * j.chunk, rows * w, slot, true, rows, w, j.chunk };
            }
        }
    }
    void run(const Job &j, Pend &pend, size_t &q)
    {
        const size_t piece = host_piece();
        if (j.after && hipStreamWaitEvent(c_.s_out, j.after, 0) != hipSuccess) { job_fail(j.J, "host layer: hipStreamWaitEvent failed"); return; }
        if (j.direct) {                                          // page-locked destination: one copy straight into it
            if (j.len && hipMemcpyAsync(j.host, j.dev, j.len, hipMemcpyDeviceToHost, c_.s_out) != hipSuccess) job_fail(j.J, "host layer: queueing a D2H copy failed");
            return;
        }
        for (size_t o = 0; o < j.len; o += piece, q++) {
            const size_t l = j.len - o < piece ? j.len - o : piece;
            const int slot = (int)(q % TRC_NSLOT);
            // (slot's previous content, piece q-3, left it two fetches ago: start() waits for the copy before it)
            if (hipMemcpyAsync(c_.pin_out[slot], j.dev + o, l, hipMemcpyDeviceToHost, c_.s_out) != hipSuccess ||
                hipEventRecord(c_.ev_out[slot], c_.s_out) != hipSuccess) { job_fail(j.J, "host layer: queueing a D2H copy failed"); return; }
            if (!fetch(pend)) return;
            pend = { j.J, j.host + o, l, slot, true };
        }
    }
    void loop()
    {
        int cur_dev = -1;
        Pend pend = { nullptr, nullptr, 0, 0, false };
        size_t q = 0;
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu_);
                if (q_.empty()) {
                    lk.unlock();
                    (void)fetch(pend);                           // nothing queued behind it: the last piece leaves its slot now
                    c_.pool_out->wait();
                    lk.lock();
                    if (q_.empty()) { idle_ = true; done_.notify_all(); cv_.wait(lk, [&] { return !q_.empty(); }); }
                }
                j = q_.front(); q_.pop_front();
            }
            if (cur_dev != c_.dev) { (void)hipSetDevice(c_.dev); cur_dev = c_.dev; }
            if (j.parts) run_streamed(j, pend, q); else run(j, pend, q);
        }
    }
    HostCtx &c_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    std::deque<Job> q_;
    bool idle_ = true;
};
// Every failure of a host-pointer call leaves through this guard: copy threads may still be writing into the caller's
// `out`, DMAs may still target the staging buffers -- nothing of the call may be in flight when it returns (the caller may
// free `out`, the next call may reallocate the pinned buffers).
struct HostDrain {
    HostCtx &c; bool ok = false;
    explicit HostDrain(HostCtx &ctx) : c(ctx) {}
    ~HostDrain()
    {
        if (ok) return;
        if (c.pool_in) c.pool_in->wait();
        if (c.out) c.out->drain();
        if (c.pool_out) c.pool_out->wait();
        if (c.s_in) (void)hipStreamSynchronize(c.s_in);
        for (int k = 0; k < c.nks; k++) if (c.s_k[k]) (void)hipStreamSynchronize(c.s_k[k]);
        if (c.s_out) (void)hipStreamSynchronize(c.s_out);
    }
};
#define TRC_MAX_DEV 64
HostCtx g_ctxs[TRC_MAX_DEV];                          // one per device: calls on the caller's current device
HostCtx g_mctxs[TRC_MAX_DEV];                         // one per POSITION of the device list (trc_set_devices): a device listed twice is two pipelines

// ---- the device list of the host-pointer calls (empty: the caller's current device) -----------------------------
std::mutex g_devs_mu;
std::vector<int> g_devs;
bool g_devs_read = false;
int devs_parse(const char *s, std::vector<int> &v)
{
    v.clear();
    if (!s || !*s) return TRC_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return TRC_E_NODEV;
    if (!strcmp(s, "all")) { for (int i = 0; i < ndev && i < TRC_MAX_DEV; i++) v.push_back(i); return TRC_OK; }
    for (const char *p = s; *p;) {
        char *e = nullptr;
        const long d = strtol(p, &e, 10);
        if (e == p || d < 0 || d >= ndev || (int)v.size() >= TRC_MAX_DEV) { v.clear(); return TRC_E_ARG; }
        v.push_back((int)d);
        p = *e == ',' ? e + 1 : e;
        if (*e && *e != ',') { v.clear(); return TRC_E_ARG; }
    }
    return TRC_OK;
}
std::vector<int> devs_get()
{
    std::lock_guard<std::mutex> lk(g_devs_mu);
    if (!g_devs_read) {
        g_devs_read = true;
        const char *e = getenv("TRC_DEVICES");
        if (e && devs_parse(e, g_devs)) fprintf(stderr, "turborc_hip: TRC_DEVICES=%s ignored (want \"all\" or a comma list of device indices)\n", e);
    }
    return g_devs;
}

int ctx_get(HostCtx *&out)
{
    int ndev = 0, dev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(TRC_E_NODEV, "no HIP device: libturborc_hip has no CPU coding path");
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= TRC_MAX_DEV) return fail(TRC_E_ARG, "device %d out of range", dev);
    out = &g_ctxs[dev];
    return TRC_OK;
}
// Coder streams per context.  Measured on the MI355X box (profiles/r06_host_pointer.txt, 100 MB, page-locked, chunk 4096): rccdf
// 27.1 / 24.9 GB/s encode / decode with one stream (the whole call one slice: copy, then code, then copy), 29.2 / 26.6 with two,
// 25.4 / 22.2 with four -- the runtime multiplexes its streams onto four hardware queues (GPU_MAX_HW_QUEUES), the two copy streams
// included, and with eight queues four streams measure like two.  Two it is: the slices are sized so that two in flight keep up
// with the link (slice_plan).
int host_streams()
{
    static const int n = [] { const char *e = getenv("TRC_HOST_STREAMS"); int v = e ? atoi(e) : 2; return v < 1 ? 1 : v > TRC_NKS_MAX ? TRC_NKS_MAX : v; }();
    return n;
}
// (the current device must be `dev`)
int ctx_init(HostCtx &c, int dev)
{
    if (c.init && c.dev == dev) return TRC_OK;
    if (c.init) {                                     // a list position that now names another device: its buffers live on the old one
        HIPCHK(hipSetDevice(c.dev));
        for (int k = 0; k < TRC_NKS_MAX; k++) { if (c.d_work[k]) (void)hipFree(c.d_work[k]); c.d_work[k] = nullptr; c.cap_work[k] = 0; }
        if (c.d_in) (void)hipFree(c.d_in);
        if (c.d_cont) (void)hipFree(c.d_cont);
        if (c.d_small) (void)hipFree(c.d_small);
        if (c.d_base) (void)hipFree(c.d_base);
        c.d_in = c.d_cont = c.d_small = c.d_base = nullptr; c.cap_in = c.cap_cont = c.cap_base = 0;
        if (c.out) c.out->drain();
        for (int i = 0; i < TRC_NSLOT; i++) {
            if (c.pin_in[i]) (void)hipHostFree(c.pin_in[i]);
            if (c.pin_out[i]) (void)hipHostFree(c.pin_out[i]);
            c.pin_in[i] = c.pin_out[i] = nullptr;
        }
        c.cap_pin = 0;
        c.ev_k.clear(); c.ev_h.clear();               // (events of the old device are left to the runtime, like its streams)
        if (c.pin_tot) (void)hipHostFree(c.pin_tot);
        if (c.pin_flags) (void)hipHostFree(c.pin_flags);
        if (c.pin_prog) (void)hipHostFree(c.pin_prog);
        c.pin_tot = nullptr; c.pin_flags = nullptr; c.pin_prog = nullptr;
        c.init = false;                               // (streams and events of the old device are left to the runtime)
        HIPCHK(hipSetDevice(dev));
    }
    c.dev = dev;
    c.nks = host_streams();
    HIPCHK(hipStreamCreateWithFlags(&c.s_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c.s_out, hipStreamNonBlocking));
    for (int k = 0; k < c.nks; k++) HIPCHK(hipStreamCreateWithFlags(&c.s_k[k], hipStreamNonBlocking));
    HIPCHK(hipMalloc((void **)&c.d_small, 65536));
    HIPCHK(hipHostMalloc((void **)&c.pin_tot, 4096 * sizeof(uint64_t)));
    HIPCHK(hipHostMalloc((void **)&c.pin_prog, 256 * sizeof(uint32_t)));
    HIPCHK(hipHostMalloc((void **)&c.pin_flags, 68 * sizeof(uint32_t)));
    for (uint32_t i = 0; i < 68; i++) c.pin_flags[i] = i < 65 ? i : 0u;                // [65]: the gate area's error word, read back behind every gated slice
    for (int i = 0; i < TRC_NSLOT; i++) {
        HIPCHK(hipEventCreateWithFlags(&c.ev_in[i], hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c.ev_out[i], hipEventDisableTiming));
    }
    HIPCHK(hipEventCreateWithFlags(&c.ev_misc, hipEventDisableTiming));
    if (!c.pool_in) { c.pool_in = new CopyPool; c.pool_out = new CopyPool; }
    if (c.out) { (void)0; }                           // (a worker of an earlier device of this list position keeps its thread: it sets the device again)
    else c.out = new OutWorker(c);
    c.init = true;
    return TRC_OK;
}
int grow(uint8_t **p, size_t *cap, size_t need)
{
    need = up256(need + TRC_PAD);
    if (*cap >= need) return TRC_OK;
    if (*p) HIPCHK(hipFree(*p));
    *p = nullptr; *cap = 0;
    size_t want = need + need / 8;
    HIPCHK(hipMalloc((void **)p, want));
    *cap = want;
    return TRC_OK;
}
// the staging slots: three per direction, one piece each
int grow_pins(HostCtx &c, bool need_pins)
{
    const size_t need = up256(host_piece() + TRC_PAD);
    if (need_pins && c.cap_pin < need) {
        if (c.out) c.out->drain();
        for (int i = 0; i < TRC_NSLOT; i++) {
            if (c.pin_in[i]) HIPCHK(hipHostFree(c.pin_in[i]));
            if (c.pin_out[i]) HIPCHK(hipHostFree(c.pin_out[i]));
            c.pin_in[i] = c.pin_out[i] = nullptr;
        }
        c.cap_pin = 0;
        for (int i = 0; i < TRC_NSLOT; i++) {
            HIPCHK(hipHostMalloc((void **)&c.pin_in[i], need));
            HIPCHK(hipHostMalloc((void **)&c.pin_out[i], need));
        }
        c.cap_pin = need;
    }
    return TRC_OK;
}
// the per-slice events of a call of `nslices` slices (created once, reused by later calls)
int grow_events(HostCtx &c, size_t nslices)
{
    while (c.ev_k.size() < nslices) {
        hipEvent_t a, b;
        HIPCHK(hipEventCreateWithFlags(&a, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&b, hipEventDisableTiming));
        c.ev_k.push_back(a); c.ev_h.push_back(b);
    }
    return TRC_OK;
}
// pageable host memory -> device, in pieces through the pin_in slots (H2D stream); the first pieces of a call are short, so that
// the link starts early.  Blocks only while the copy threads stage.
bool push_in(HostCtx &c, HostJob &J, uint8_t *dev, const uint8_t *host, size_t len);
// Is [p, p + len) page-locked host memory the GPU can address (hipHostMalloc, or registered with hipHostRegister /
// trc_host_pin)?  Then a host-pointer call moves its bytes by DMA straight from / to the caller's buffer; pageable
// buffers go through the pinned staging slots and the copy threads.
bool host_is_pinned(const void *p, size_t len)
{
    static const bool off = getenv("TRC_HOST_NO_DIRECT") != nullptr;      // tuning aid: always stage
    if (off || !p || !len) return false;
    const char *ends[2] = { (const char *)p, (const char *)p + len - 1 };
    for (const char *q : ends) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}
// cdfnum = index of the terminating 1<<15 (cdf is strictly increasing from 0)
int host_cdfnum(const cdf_t *cdf)
{
    if (!cdf || cdf[0] != 0) return -1;
    for (int i = 1; i <= 256; i++) {
        if (cdf[i] == TRC_PROB_ONE_HOST) return i;
        if (cdf[i] <= cdf[i - 1] || cdf[i] > TRC_PROB_ONE_HOST) return -1;
    }
    return -1;
}
// Slice plan of one shard of a host-pointer call: whole groups of 64 chunks.  A slice is sized for the copies -- ~16 MB of input
// (8-32 MB measure alike on the MI355X box, 4 MB throughout is 30 % slower: per-slice synchronisation) -- and, round 6, for the
// coder streams: `nks` slices in flight must code at least as fast as the link delivers, and a slice takes ONE WAVE'S time
// however few chunks it has (TrcCodec::wave_ns per chunk byte).  So slice bytes >= 1.2 x 50 GB/s x (one wave's time) / nks, at most one
// residency round of the coder and 256 MB of staging.  TRC_HOST_SLICE overrides the byte target for every coder.  The plan
// ramps up from 1/8 of the slice at the start and down to 1/8 at the end: the first H2D copy and the last D2H copy + unstaging
// are the part of the pipeline nothing overlaps with, so they are kept short.
// first[i] = first chunk of slice i (relative to the shard), first[nsl] = nchunks; returns the largest slice in chunks.
size_t slice_plan(int codec, uint32_t chunk, size_t nchunks, int nks, std::vector<size_t> &first)
{
    static const size_t forced = getenv("TRC_HOST_SLICE") ? (size_t)strtoull(getenv("TRC_HOST_SLICE"), 0, 10) : 0;
    static const bool no_ramp = getenv("TRC_HOST_NO_RAMP") != nullptr;
    if (nks < 1) nks = 1;
    const TrcCodec &r = codec_row(codec);
    const size_t ngroups = (nchunks + 63) / 64;
    const double wave_s = 1e-9 * r.wave_ns * chunk;                                    // one wave of this coder at this chunk
    size_t target = forced ? forced : (size_t)16 << 20;
    bool equal = false;                                                                // equal slices, no ramps: every slice costs a wave's time on its stream
    if (!forced) {
        const size_t keep_up = (size_t)(1.2 * 50e9 * wave_s / nks);
        if (keep_up > target) { target = keep_up; equal = true; }
        const size_t round = (size_t)r.round_lanes * chunk;                            // more than one residency round per slice buys nothing
        if (target > round) target = round;
        if (target > ((size_t)256 << 20)) target = (size_t)256 << 20;
    }
    size_t groups = target / ((size_t)chunk * 64);
    // an order-1 coder keeps its model per chunk of a slice in every workspace (136 KiB: anscdf1, rccs; 64 KiB: rcxs): 1 GiB of models = 7 700 chunks = 31 MB
    // slices at chunk 4096 (ADVICE r3: a 65 536-chunk slice would ask for 9 GB)
    // (the word coders: 136.5 KiB .. 2.26 MiB per chunk; 1 GiB of them is 7 groups of rcc2s32, 7.3 MB at chunk 16384)
    const size_t mpc = r.slice_model ? r.slice_model(r) : 0;
    if (mpc && !forced && groups > ((size_t)1 << 30) / (64u * mpc)) groups = ((size_t)1 << 30) / (64u * mpc);
    if (groups < 1) groups = 1;
    while ((ngroups + groups - 1) / groups > TRC_MAX_SLICES) groups *= 2;              // the totals area holds 4096 slices
    if (equal) {                                                                       // a short last slice would cost its stream a whole wave's time: spread the groups evenly
        size_t m = (ngroups + groups / 2) / groups;
        if (m < 1) m = 1;
        groups = (ngroups + m - 1) / m;
    }
    const size_t per = groups * 64;
    auto part = [&](int sh) { size_t g = groups >> sh; return (g < 1 ? 1 : g) * 64; };
    first.clear();
    size_t c = 0;
    std::vector<size_t> tail;
    size_t left = nchunks;
    size_t ramp_chunks = 0;
    for (int sh = 3; sh >= 1; sh--) ramp_chunks += part(sh);                // part() never goes below one group: with small slice targets the
    // ramps are longer than 7/8 of a slice each -- count what they really take.  And a ramp slice costs its coder stream a wave's time
    // like any other: ramps only while the streams would still be idle half of the call (static rANS yes, the range coders no)
    const double slices = (double)(nchunks / per + 7), link_s = (double)nchunks * chunk / 50e9;
    const bool ramp = !no_ramp && !equal && (forced || slices / nks * wave_s <= 0.5 * link_s);
    if (ramp && nchunks > 4 * per && nchunks > 2 * ramp_chunks + per) {
        for (int sh = 3; sh >= 1; sh--) { first.push_back(c); c += part(sh); }   // up: per/8, per/4, per/2; the same coming down
        for (int sh = 3; sh >= 1; sh--) tail.push_back(part(sh));
        left = nchunks - 2 * ramp_chunks;
        left = (left + 63) / 64 * 64;                                       // (every slice starts on a group boundary: the last one takes what is left)
    }
    size_t tail_sum = 0;
    for (size_t v : tail) tail_sum += v;
    if (c + left + tail_sum > nchunks + 63) left = nchunks - c - tail_sum;   // (cannot happen: left was rounded up by < 64)
    for (size_t done = 0; done < left; done += per) first.push_back(c + done);
    c += left;
    for (size_t k = tail.size(); k-- > 0;) { if (c >= nchunks) break; first.push_back(c); c += tail[k]; }      // largest first: per/2, per/4, per/8
    first.push_back(nchunks);
    const size_t all = ngroups * 64;                                        // a short call sizes its staging slots and workspace by what it has
    return per < all ? per : all;
}
// The plan of one shard (whole chunks C0 .. C1 of a call on one pipeline): its slices -- launches -- and, for the coders that support
// it, the parts of a striped input (encode) or streamed output (decode).
struct ShardPlan {
    std::vector<size_t> sc;      // first chunk of every slice, relative to the shard; sc[nsl] = the shard's chunks
    size_t nsl = 0, per = 0;     // slices; the largest slice in chunks
    size_t part = 0, K = 0;      // gated: bytes of a chunk per pass, passes
    bool gated = false;          // encode: striped input behind arrival gates; decode: streamed output behind progress flags
};
// ENCODE, striped input (the coders whose encoder waits at an arrival gate: trc_io.h, WaveChunks::gate; trc_gate_ok).  A slice is ONE
// launch, started while its input is still on the link, and the input comes in K passes -- pass k = bytes [k part, (k + 1) part) of every
// chunk, one 2-D copy (rows of >= 1 KB move at the link's full rate both ways: scripts/probe/pcie_2d.cpp) -- each followed by a 4-byte
// copy that opens the gate for it.  The waves code part k while part k + 1 is on the link: the call lasts about max(link / K + wave,
// link + wave / K) instead of link + wave.
//   PAGE-LOCKED input only.  A waiting kernel must never have anything it needs queued BEHIND it: where two of the process's streams
//   share a hardware queue (four queues, any number of streams) a small copy -- a flag, a ragged last chunk: blit KERNELS -- issued after
//   the launch sits behind the waiting kernel for good (scripts/soak_host_layer.py found it: the wait timed out, the call fell back).
//   With page-locked input every copy of a slice is queued BEFORE its kernel, which rules that out by construction, for any number of
//   pipelines (A's flags behind B's kernel and B's flags behind A's kernel would need each kernel to precede its own flags).
//   Pageable input would have to be staged while the kernel waits -- copies behind the launch -- and gained little when measured (24
//   against 22-25 GB/s): it takes the slice pipeline.
//   SLICES of its own only when the shard is long: a slice's payload then travels back while the next slice's input comes in.  A
//   slice's kernels last at least one wave's time from the arrival of its first pass, and slices j and j + 2 share a coder stream, so a
//   slice's transfer must take longer than a wave (1.25 x): 100 MB of `rccdf` at chunk 4096 (link 1.8 ms, wave 1.35 ms) is ONE launch
//   -- four slices measured 27.5 GB/s against 34.7, each kernel waiting for the one before it on its stream
//   (profiles/r06_host_striped_trace.txt) -- 1 GB at chunk 16 384 (18 ms, 6.7 ms) is two.  And a launch never exceeds one residency
//   round of the coder: the waves of a second round would start when the first round's end.
// DECODE, streamed output (the coders whose decoder reports its progress: WaveChunks::prog; trc_prog_ok): the waves store part k of
// every chunk write-through, count themselves, and the last one sets a flag in page-locked host memory; the context's out-worker polls
// the flags and fetches part k of every chunk (a 2-D copy) while the waves decode part k + 1.  A decode then lasts about payload time +
// wave / K + link instead of payload + wave + link.  One launch per residency round (the waves of a second round would finish their
// FIRST part only after the first round's last).  Above 512 MB a decode is the link's: the slice pipeline, which sends the next
// slice's payload up while this one decodes, measured as fast or faster (anscdf 1 GB: 41.6 against 36-38 GB/s streamed); pageable
// output: up to 256 MB, and at most four passes (it is scattered row by row by the copy threads: 1 GB at chunk 16 384 in sixteen
// passes of 1 KB rows decoded at 20.7 GB/s against 32.2 through the slice pipeline).
// Both: chunks that are multiples of 128 bytes from 2048 up (no cache line holds bytes of two passes), parts of chunk / 8, at least
// 1 KB (1 GB at chunk 16 384: sixteen passes of 1 KB measured below eight of 2 KB).  Everything else: slice_plan.
void plan_shard(int codec, uint32_t chunk, size_t nch, size_t sbytes, int nks, bool decode, bool direct, bool no_gates, ShardPlan &P)
{
    static const bool no_stripe = getenv("TRC_HOST_NO_STRIPE") != nullptr;
    P = ShardPlan();
    if (!nch) return;
    const bool shape = sbytes >= chunk && !no_stripe && (chunk & 127u) == 0 && chunk >= 2048u;
    const bool want = decode ? shape && trc_prog_ok(codec) && sbytes <= (direct ? (size_t)512 << 20 : (size_t)256 << 20)
                             : shape && !no_gates && trc_gate_ok(codec) && direct;
    if (want) {
        size_t part = ((chunk + 7u) / 8u + 127u) & ~(size_t)127u;
        if (part < 1024u) part = 1024u;
        if (decode && !direct && part < (((size_t)chunk / 4u + 127u) & ~(size_t)127u)) part = ((size_t)chunk / 4u + 127u) & ~(size_t)127u;
        if (host_part_env() >= 128u && (chunk + host_part_env() - 1) / host_part_env() <= 16u) part = host_part_env();     // (16 gate values / flags per launch)
        const size_t ngroups = (nch + 63) / 64, round_groups = codec_row(codec).round_lanes / 64u;
        size_t m = (ngroups + round_groups - 1) / round_groups;
        if (!decode) {
            const double link_s = (double)sbytes / 50e9, wave_s = 1e-9 * codec_row(codec).wave_ns * chunk;
            const size_t by_time = (size_t)(link_s / (1.25 * wave_s));
            if (m < by_time) m = by_time;
        }
        m = m < 1 ? 1 : m > 16 ? 16 : m;
        size_t g = (ngroups + m - 1) / m;
        if (g > round_groups) g = round_groups;
        if (g < 1) g = 1;
        for (size_t c0 = 0; c0 < nch; c0 += g * 64) P.sc.push_back(c0);
        if (P.sc.size() <= 16) {                                                      // (16 sets of gates / counters and flags: longer calls take the slice pipeline)
            P.sc.push_back(nch); P.nsl = P.sc.size() - 1;
            P.per = g * 64 < ngroups * 64 ? g * 64 : ngroups * 64;
            P.part = part; P.K = (chunk + part - 1) / part; P.gated = true;
            return;
        }
        P.sc.clear();
    }
    P.per = slice_plan(codec, chunk, nch, nks, P.sc);
    P.nsl = P.sc.size() - 1;
}
// shards of a call over `ndev` pipelines: contiguous ranges of whole groups, as even as the groups allow; a pipeline may get nothing
void shard_plan(size_t nchunks, int ndev, std::vector<size_t> &first)
{
    const size_t ngroups = (nchunks + 63) / 64;
    first.assign((size_t)ndev + 1, nchunks);
    for (int s = 0; s < ndev; s++) {
        const size_t g = ngroups * (size_t)s / (size_t)ndev;
        first[s] = g * 64 < nchunks ? g * 64 : nchunks;
    }
    first[0] = 0;
}

// What the shards of one call share.  Errors of a worker thread travel through `err` (trc_last_error is per thread).
struct HostJob {
    int codec = 0; uint32_t chunk = 0; int cdfnum = 0; const cdf_t *cdf = nullptr;
    unsigned prm = 0;                     // "ss" coders: TRC_SS_PRM of the call (they have no CDF: cdfnum stays 0), else 0
    const uint8_t *in = nullptr; uint8_t *out = nullptr;
    size_t n = 0;                         // plain bytes (encode: inlen, decode: outlen)
    size_t nchunks = 0, dir = 0, hdrsz = sizeof(trc_container_hdr);
    size_t lim = 0;                       // encode: payload bytes at which the call turns raw
    bool in_direct = false, out_direct = false;
    std::vector<size_t> shard;            // first chunk of every shard, [nshard] = nchunks
    std::vector<uint64_t> gcum;           // decode: payload offset of every group of 64 chunks, [ngroups] = total
    std::mutex mu; std::condition_variable cv;
    std::vector<long long> total;         // encode: payload bytes of shard s once all its kernels are done, -1 before
    bool raw = false, failed = false;
    bool gate_timeout = false;            // encode: a striped slice's wait at its arrival gate timed out (the call is repeated without gates)
    bool no_gates = false;                // encode: take the slice pipeline for every coder
    std::string err;
    void fail_with(const char *msg)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!failed) { failed = true; err = msg; }
        cv.notify_all();
    }
};
void job_fail(HostJob *J, const char *msg) { if (J) J->fail_with(msg); }
bool job_failed(HostJob *J) { if (!J) return false; std::lock_guard<std::mutex> lk(J->mu); return J->failed; }
#define SCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { char m_[300]; snprintf(m_, sizeof m_, "%s -> %s", #x, hipGetErrorString(e_)); J.fail_with(m_); return false; } } while (0)
#define SFAIL(msg) do { J.fail_with(msg); return false; } while (0)

bool push_in(HostCtx &c, HostJob &J, uint8_t *dev, const uint8_t *host, size_t len)
{
    const size_t piece = host_piece();
    for (size_t o = 0; o < len; c.qin++) {
        size_t want = c.qin < 3 ? piece >> (3 - c.qin) : piece;                     // 1/8, 1/4, 1/2 of a piece, then whole pieces
        if (want < 65536) want = 65536;
        const size_t l = len - o < want ? len - o : want;
        const int k = (int)(c.qin % TRC_NSLOT);
        if (c.qin >= TRC_NSLOT) SCHK(hipEventSynchronize(c.ev_in[k]));               // slot free: its last H2D is done
        c.pool_in->copy(c.pin_in[k], host + o, l);
        SCHK(hipMemcpyAsync(dev + o, c.pin_in[k], l, hipMemcpyHostToDevice, c.s_in));
        SCHK(hipEventRecord(c.ev_in[k], c.s_in));
        o += l;
    }
    return true;
}

// ---- one shard of a host-pointer encode on one context (the current device is c.dev, c.mu is held) --------------
bool encode_shard(HostCtx &c, HostJob &J, int s)
{
    HostDrain guard(c);
    const uint32_t chunk = J.chunk;
    const int codec = J.codec, cdfnum = J.cdfnum;
    const size_t C0 = J.shard[s], C1 = J.shard[s + 1], nch = C1 - C0;
    const size_t b0 = C0 * (size_t)chunk, b1 = C1 == J.nchunks ? J.n : C1 * (size_t)chunk, sbytes = b1 - b0;
    size_t shard_total = 0;
    ShardPlan P;
    plan_shard(codec, chunk, nch, sbytes, c.nks, false, J.in_direct, J.no_gates, P);
    const std::vector<size_t> &sc = P.sc;
    const size_t nsl = P.nsl, per = P.per, part = P.part, K = P.K;
    const bool gated = P.gated;
    const int nks = nsl < (size_t)c.nks ? (int)(nsl ? nsl : 1) : c.nks;
    const size_t slice_bytes = per * (size_t)chunk;
    const size_t dirsz = up256(4 * nch + 256);
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    uint64_t *d_tot = (uint64_t *)(c.d_small + 2048);
    uint32_t *d_clen = nullptr;
    uint8_t *d_payload = nullptr;
    int flags = 0;
    c.qin = 0;
    if (nch) {
        const size_t wb = trc_work_bytes(codec, slice_bytes < sbytes ? slice_bytes : sbytes, chunk);
        if (grow(&c.d_in, &c.cap_in, sbytes) || grow(&c.d_cont, &c.cap_cont, dirsz + sbytes + nsl * TRC_PAD + 64) ||
            grow_pins(c, !J.in_direct || !J.out_direct) || grow_events(c, nsl)) SFAIL(trc_last_error());
        for (int k = 0; k < nks; k++) if (grow(&c.d_work[k], &c.cap_work[k], wb)) SFAIL(trc_last_error());
        d_clen = (uint32_t *)c.d_cont;
        d_payload = c.d_cont + dirsz;
        if (cdfnum) {
            SCHK(hipMemcpyAsync(d_cdf, J.cdf, (cdfnum + 1) * sizeof(cdf_t), hipMemcpyHostToDevice, c.s_k[0]));
            SCHK(hipEventRecord(c.ev_misc, c.s_k[0]));
            for (int k = 0; k < nks; k++) {
                if (k) SCHK(hipStreamWaitEvent(c.s_k[k], c.ev_misc, 0));
                if (trc_tables_dev(d_cdf, (unsigned)cdfnum, c.d_work[k], c.cap_work[k], c.s_k[k])) SFAIL(trc_last_error());
            }
            flags = TRC_TABLES_READY;
        }
    }
    auto slice_off = [&](size_t i) { return sc[i] * (size_t)chunk; };                    // relative to the shard
    auto slice_len = [&](size_t i) { const size_t o = slice_off(i), e = i + 1 == nsl ? sbytes : slice_off(i + 1); return e - o; };
    // every slice has a payload region of its own (its input length + slack: the gather stores whole segments), so slices are coded
    // without knowing how much the ones before them produced
    auto slice_pay = [&](size_t i) { return d_payload + slice_off(i) + i * (size_t)TRC_PAD; };
    std::vector<size_t> tot(nsl, 0);
    // H2D of slice j (pageable: staged piece by piece), then its coder kernels on stream j % nks
    auto produce = [&](size_t j) -> bool {
        const int ks = (int)(j % (size_t)nks);
        const size_t o = slice_off(j), l = slice_len(j);
        if (J.in_direct) SCHK(hipMemcpyAsync(c.d_in + o, J.in + b0 + o, l, hipMemcpyHostToDevice, c.s_in));
        else if (!push_in(c, J, c.d_in + o, J.in + b0 + o, l)) return false;
        SCHK(hipEventRecord(c.ev_h[j], c.s_in));
        SCHK(hipStreamWaitEvent(c.s_k[ks], c.ev_h[j], 0));
        if (trc_encode_dev(codec | flags, c.d_in + o, l, chunk, cdfnum ? d_cdf : nullptr, cdfnum ? (unsigned)cdfnum : J.prm, d_clen + sc[j], slice_pay(j),
                           d_tot + j, c.d_work[ks], c.cap_work[ks], c.s_k[ks])) SFAIL(trc_last_error());
        SCHK(hipMemcpyAsync(c.pin_tot + j, d_tot + j, 8, hipMemcpyDeviceToHost, c.s_k[ks]));
        SCHK(hipEventRecord(c.ev_k[j], c.s_k[ks]));
        return true;
    };
    // slice j as one launch behind its arrival gate (see above): gate word j, passes over the slice's own rows
    uint32_t *const gates = (uint32_t *)(c.d_small + 49152);
    auto produce_striped = [&](size_t j) -> bool {
        const int ks = (int)(j % (size_t)nks);
        const size_t o = slice_off(j), l = slice_len(j), nfull = l / chunk;             // whole chunks of the slice (a ragged last one goes up with pass 0)
        if (j == 0) {
            c.pin_flags[65] = 0;
            SCHK(hipMemsetAsync(gates, 0, 256, c.s_in));
            SCHK(hipEventRecord(c.ev_h[0], c.s_in));
        }
        auto launch = [&]() -> bool {
            SCHK(hipStreamWaitEvent(c.s_k[ks], c.ev_h[0], 0));                         // behind the gates' reset, not behind the input
            trc_gate_tls = { gates + j, (uint32_t)part };
            const int rc = trc_encode_dev(codec | flags, c.d_in + o, l, chunk, cdfnum ? d_cdf : nullptr, cdfnum ? (unsigned)cdfnum : J.prm, d_clen + sc[j], slice_pay(j),
                                          d_tot + j, c.d_work[ks], c.cap_work[ks], c.s_k[ks]);
            trc_gate_tls = { nullptr, 0 };
            if (rc) SFAIL(trc_last_error());
            SCHK(hipMemcpyAsync(c.pin_tot + j, d_tot + j, 8, hipMemcpyDeviceToHost, c.s_k[ks]));
            SCHK(hipMemcpyAsync(c.pin_flags + 65, gates + 63, 4, hipMemcpyDeviceToHost, c.s_k[ks]));      // "a wait at the gate timed out"
            SCHK(hipEventRecord(c.ev_k[j], c.s_k[ks]));
            return true;
        };
        // every copy of the slice, then its kernel (see `striped` above)
        const uint8_t *src = J.in + b0 + o;
        uint8_t *dst = c.d_in + o;
        for (size_t k = 0; k < K; k++) {
            const size_t w = chunk - k * part < part ? chunk - k * part : part;
            if (nfull) SCHK(hipMemcpy2DAsync(dst + k * part, chunk, src + k * part, chunk, w, nfull, hipMemcpyHostToDevice, c.s_in));
            if (k == 0 && l > nfull * chunk)                                          // the ragged last chunk, whole, with the first pass
                SCHK(hipMemcpyAsync(dst + nfull * chunk, src + nfull * chunk, l - nfull * chunk, hipMemcpyHostToDevice, c.s_in));
            static const bool sabotage = getenv("TRC_HOST_GATE_SABOTAGE") != nullptr;                // tests only: the last pass never opens its gate
            if (sabotage && k + 1 == K && !J.no_gates) continue;
            SCHK(hipMemcpyAsync(gates + j, c.pin_flags + k + 1, 4, hipMemcpyHostToDevice, c.s_in));  // pass k has landed: the gate opens for it
        }
        return launch();
    };
    // the way back of slice i, whose size and place are known: page-locked `out`: two D2H copies straight into it; pageable: the
    // context's out-worker takes the directory slice and the payload through the staging slots
    size_t ppos = 0;                                                        // payload position in `out` of the next slice to go back (shard base included)
    auto drain = [&](size_t i) -> bool {
        { std::lock_guard<std::mutex> lk(J.mu); if (J.raw || ppos + tot[i] >= J.lim) { J.raw = true; return true; } }   // nothing more is written to `out`: the call ends in the raw copy
        const size_t nc = sc[i + 1] - sc[i];
        uint8_t *o_dir = J.out + J.hdrsz + 4 * (C0 + sc[i]), *o_pay = J.out + J.hdrsz + J.dir + ppos;
        if (J.out_direct) {
            SCHK(hipStreamWaitEvent(c.s_out, c.ev_k[i], 0));
            SCHK(hipMemcpyAsync(o_dir, d_clen + sc[i], 4 * nc, hipMemcpyDeviceToHost, c.s_out));
            SCHK(hipMemcpyAsync(o_pay, slice_pay(i), tot[i], hipMemcpyDeviceToHost, c.s_out));
        } else {
            c.out->submit({ &J, (const uint8_t *)(d_clen + sc[i]), o_dir, 4 * nc, c.ev_k[i] });
            c.out->submit({ &J, slice_pay(i), o_pay, tot[i], nullptr });
        }
        ppos += tot[i];
        return true;
    };
    // Shard 0 knows where its payload goes (the start of the payload area) and sends every slice back as soon as its size is
    // read.  A later shard learns its base when the shards before it have finished coding; its slices wait on the device till then.
    size_t i = 0, j = 0;                                                    // next slice to read the size of / to launch
    while (i < nsl) {
        bool launch = j < nsl && j < i + TRC_NKEV - 1;
        if (launch && j > i) {                                              // something is in flight: a finished slice goes back before the next one is staged
            const hipError_t q = hipEventQuery(c.ev_k[i]);
            if (q == hipSuccess) launch = false; else if (q != hipErrorNotReady) SCHK(q); else (void)hipGetLastError();     // "not ready" is no error of this call
        }
        { std::lock_guard<std::mutex> lk(J.mu); if (J.failed) return false; }
        if (launch) { if (!(gated ? produce_striped(j) : produce(j))) return false; j++; continue; }
        SCHK(hipEventSynchronize(c.ev_k[i]));
        if (gated && c.pin_flags[65]) {                                     // a pass never opened its gate: what the kernels produced is garbage
            { std::lock_guard<std::mutex> lk(J.mu); J.gate_timeout = true; }
            char m_[320];
            snprintf(m_, sizeof m_, "an arrival gate timed out (a copy of this call queued behind a waiting coder kernel?): codec %d, shard %d of %zu, slice %zu of %zu, "
                     "%zu bytes, chunk %u, %zu passes of %zu bytes, input %s", codec, s, J.shard.size() - 1, i, nsl, sbytes, chunk, K, part, J.in_direct ? "page-locked" : "pageable");
            SFAIL(m_);
        }
        tot[i] = (size_t)c.pin_tot[i];
        shard_total += tot[i];
        if (s == 0 && !drain(i)) return false;
        i++;
    }
    {
        std::unique_lock<std::mutex> lk(J.mu);
        J.total[s] = (long long)shard_total;
        J.cv.notify_all();
        if (s > 0) {
            J.cv.wait(lk, [&] { if (J.failed) return true; for (int t = 0; t < s; t++) if (J.total[t] < 0) return false; return true; });
            if (J.failed) return false;
            for (int t = 0; t < s; t++) ppos += (size_t)J.total[t];
        }
    }
    if (s > 0) for (size_t k = 0; k < nsl; k++) if (!drain(k)) return false;
    c.out->drain();
    SCHK(hipStreamSynchronize(c.s_in));
    if (J.out_direct) SCHK(hipStreamSynchronize(c.s_out));
    { std::lock_guard<std::mutex> lk(J.mu); if (J.failed) return false; }
    guard.ok = true;                                                        // everything of this shard has landed
    return true;
}

// ---- one shard of a host-pointer decode ------------------------------------------------------------------------
bool decode_shard(HostCtx &c, HostJob &J, int s)
{
    HostDrain guard(c);
    const uint32_t chunk = J.chunk;
    const int codec = J.codec, cdfnum = J.cdfnum;
    const size_t C0 = J.shard[s], C1 = J.shard[s + 1], nch = C1 - C0;
    if (!nch) { guard.ok = true; return true; }
    const size_t b0 = C0 * (size_t)chunk, b1 = C1 == J.nchunks ? J.n : C1 * (size_t)chunk, sbytes = b1 - b0;
    ShardPlan P;
    plan_shard(codec, chunk, nch, sbytes, c.nks, true, J.out_direct, false, P);
    const std::vector<size_t> &sc = P.sc;
    const size_t nsl = P.nsl, per = P.per, part = P.part, K = P.K;
    const bool streaming = P.gated;
    const int nks = nsl < (size_t)c.nks ? (int)nsl : c.nks;
    const size_t slice_bytes = per * (size_t)chunk;
    const size_t wb = trc_work_bytes(codec, slice_bytes < sbytes ? slice_bytes : sbytes, chunk);
    const size_t dirsz = up256(4 * nch + 256);
    auto gpos = [&](size_t rel_chunk) { const size_t g = (C0 + rel_chunk + 63) / 64; return (size_t)J.gcum[g < J.gcum.size() ? g : J.gcum.size() - 1]; };   // payload offset of a slice boundary (a group boundary, or the end)
    const size_t p0 = gpos(0), spay = gpos(nch) - p0;
    c.qin = 0;
    if (grow(&c.d_in, &c.cap_in, sbytes) || grow(&c.d_cont, &c.cap_cont, dirsz + spay + 2 * nsl + 64) ||
        grow_pins(c, !J.in_direct || !J.out_direct) || grow_events(c, nsl)) SFAIL(trc_last_error());
    for (int k = 0; k < nks; k++) if (grow(&c.d_work[k], &c.cap_work[k], wb)) SFAIL(trc_last_error());
    uint16_t *d_cdf = (uint16_t *)c.d_small;
    uint32_t *d_clen = (uint32_t *)c.d_cont;
    uint8_t *d_payload = c.d_cont + dirsz;
    int flags = 0;
    if (cdfnum) {
        SCHK(hipMemcpyAsync(d_cdf, J.cdf, (cdfnum + 1) * sizeof(cdf_t), hipMemcpyHostToDevice, c.s_k[0]));
        SCHK(hipEventRecord(c.ev_misc, c.s_k[0]));
        for (int k = 0; k < nks; k++) {
            if (k) SCHK(hipStreamWaitEvent(c.s_k[k], c.ev_misc, 0));
            if (trc_tables_dev(d_cdf, (unsigned)cdfnum, c.d_work[k], c.cap_work[k], c.s_k[k])) SFAIL(trc_last_error());
        }
        flags = TRC_TABLES_READY;
    }
    const uint8_t *in_dir = J.in + J.hdrsz, *in_pay = J.in + J.hdrsz + J.dir;
    for (size_t i = 0; i < nsl; i++) if (sc[i] & 63) SFAIL("slice plan: a slice does not start on a group boundary");       // gpos() below
    auto slice_off = [&](size_t i) { return sc[i] * (size_t)chunk; };
    auto slice_len = [&](size_t i) { const size_t o = slice_off(i), e = i + 1 == nsl ? sbytes : slice_off(i + 1); return e - o; };
    // (payload offsets are odd only for corrupt directories; the device layer wants 2-byte alignment: every slice's own offset is kept even)
    auto slice_pay = [&](size_t i) { return d_payload + ((gpos(sc[i]) - p0 + 1) & ~(size_t)1) + 2 * i; };
    // Slice i: its directory slice and payload go up (pageable: staged in pieces), its kernels run on stream i % nks, its bytes come
    // back (page-locked `out`: one D2H copy; pageable: the context's out-worker).  Everything is queued without waiting for a kernel:
    // the host only ever waits for a staging slot.
    for (size_t i = 0; i < nsl; i++) {
        const int ks = (int)(i % (size_t)nks);
        const size_t o = slice_off(i), l = slice_len(i), c0 = sc[i], nc = sc[i + 1] - c0, po = gpos(c0), pl = gpos(sc[i + 1]) - po;
        { std::lock_guard<std::mutex> lk(J.mu); if (J.failed) return false; }
        if (J.in_direct) {
            SCHK(hipMemcpyAsync(d_clen + c0, in_dir + 4 * (C0 + c0), 4 * nc, hipMemcpyHostToDevice, c.s_in));
            SCHK(hipMemcpyAsync(slice_pay(i), in_pay + po, pl, hipMemcpyHostToDevice, c.s_in));
        } else if (!push_in(c, J, (uint8_t *)(d_clen + c0), in_dir + 4 * (C0 + c0), 4 * nc) || !push_in(c, J, slice_pay(i), in_pay + po, pl)) return false;
        SCHK(hipEventRecord(c.ev_h[i], c.s_in));
        SCHK(hipStreamWaitEvent(c.s_k[ks], c.ev_h[i], 0));
        if (streaming) {
            uint32_t *counters = (uint32_t *)(c.d_small + 49152 + 256) + 16 * i;
            volatile uint32_t *pflags = c.pin_prog + 16 * i;
            for (size_t k = 0; k < 16; k++) pflags[k] = 0;
            SCHK(hipMemsetAsync(counters, 0, 64, c.s_k[ks]));
            trc_prog_tls = { counters, c.pin_prog + 16 * i, (uint32_t)part };
            const int rc = trc_decode_dev(codec | flags, d_clen + c0, slice_pay(i), l, chunk, cdfnum ? d_cdf : nullptr, cdfnum ? (unsigned)cdfnum : J.prm,
                                          c.d_in + o, c.d_work[ks], c.cap_work[ks], c.s_k[ks]);
            trc_prog_tls = { nullptr, nullptr, 0 };
            if (rc) SFAIL(trc_last_error());
            SCHK(hipEventRecord(c.ev_k[i], c.s_k[ks]));
            const size_t nfull = l / chunk;
            OutWorker::Job sj = { &J, c.d_in + o, J.out + b0 + o, 0, nullptr };
            sj.parts = K; sj.part = part; sj.chunk = chunk; sj.rows = nfull; sj.flags = pflags; sj.direct = J.out_direct;
            if (nfull) c.out->submit(sj);
            if (l > nfull * chunk) {                                                  // the ragged last chunk: whole, behind the kernel's end
                OutWorker::Job tj = { &J, c.d_in + o + nfull * chunk, J.out + b0 + o + nfull * chunk, l - nfull * chunk, c.ev_k[i] };
                tj.direct = J.out_direct;
                c.out->submit(tj);
            }
            continue;
        }
        if (trc_decode_dev(codec | flags, d_clen + c0, slice_pay(i), l, chunk, cdfnum ? d_cdf : nullptr, cdfnum ? (unsigned)cdfnum : J.prm,
                           c.d_in + o, c.d_work[ks], c.cap_work[ks], c.s_k[ks])) SFAIL(trc_last_error());
        SCHK(hipEventRecord(c.ev_k[i], c.s_k[ks]));
        if (J.out_direct) {
            SCHK(hipStreamWaitEvent(c.s_out, c.ev_k[i], 0));
            SCHK(hipMemcpyAsync(J.out + b0 + o, c.d_in + o, l, hipMemcpyDeviceToHost, c.s_out));
        } else c.out->submit({ &J, c.d_in + o, J.out + b0 + o, l, c.ev_k[i] });
    }
    c.out->drain();
    SCHK(hipStreamSynchronize(c.s_in));
    if (J.out_direct) SCHK(hipStreamSynchronize(c.s_out));
    { std::lock_guard<std::mutex> lk(J.mu); if (J.failed) return false; }
    guard.ok = true;
    return true;
}

// run every shard of a job: shard 0 on the calling thread, the others on threads of their own; one context per shard
// (the caller's current device, or the positions of the device list)
bool run_shards(HostJob &J, const std::vector<int> &devs, bool decode)
{
    const int nshard = (int)J.shard.size() - 1;
    auto one = [&](HostCtx &c, int dev, int s) {
        std::lock_guard<std::mutex> lk(c.mu);
        if (hipSetDevice(dev) != hipSuccess) { J.fail_with("hipSetDevice failed"); return; }
        if (ctx_init(c, dev)) { J.fail_with(trc_last_error()); return; }
        if (!(decode ? decode_shard(c, J, s) : encode_shard(c, J, s))) J.fail_with("shard failed");      // (keeps the first message)
    };
    if (devs.empty()) {                                                     // one pipeline on the caller's current device
        HostCtx *cp = nullptr;
        if (ctx_get(cp)) { J.fail_with(trc_last_error()); return false; }
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) { J.fail_with("hipGetDevice failed"); return false; }
        one(*cp, dev, 0);
        return !J.failed;
    }
    static std::mutex multi_mu;                                             // calls over the device list take their turns: a shard waits for the shards before it
    std::lock_guard<std::mutex> mlk(multi_mu);
    int prev = 0;
    (void)hipGetDevice(&prev);
    std::vector<std::thread> th;
    for (int s = 1; s < nshard; s++) th.emplace_back([&, s] { one(g_mctxs[s], devs[s], s); });
    one(g_mctxs[0], devs[0], 0);
    for (auto &t : th) t.join();
    (void)hipSetDevice(prev);
    return !J.failed;
}
}  // namespace

extern "C" int trc_set_devices(const int *devs, int ndev)
{
    if (ndev < 0 || ndev > TRC_MAX_DEV || (ndev && !devs)) return fail(TRC_E_ARG, "set_devices: bad arguments");
    int have = 0;
    if (ndev && (hipGetDeviceCount(&have) != hipSuccess || have < 1)) return fail(TRC_E_NODEV, "no HIP device");
    for (int i = 0; i < ndev; i++) if (devs[i] < 0 || devs[i] >= have) return fail(TRC_E_ARG, "set_devices: device %d of %d", devs[i], have);
    std::lock_guard<std::mutex> lk(g_devs_mu);
    g_devs.assign(devs, devs + ndev);
    g_devs_read = true;
    return TRC_OK;
}
// the plan of a host-pointer call on ONE pipeline, for tests and diagnostics (needs no device)
extern "C" int trc_host_plan(int codec, size_t n, uint32_t chunk, int decode, int page_locked, size_t *first_chunk, int cap, uint32_t *part_bytes)
{
    if (!codec_ok(codec) || !n) return fail(TRC_E_ARG, "host_plan: bad arguments");
    if (!chunk) chunk = trc_auto_chunk_codec(codec, n);
    if (!chunk_ok(chunk)) return fail(TRC_E_ARG, "host_plan: chunk %u", chunk);
    ShardPlan P;
    plan_shard(codec, chunk, (n + chunk - 1) / chunk, n, host_streams(), decode != 0, page_locked != 0, false, P);
    for (size_t i = 0; i <= P.nsl && (int)i < cap; i++) first_chunk[i] = P.sc[i];
    if (part_bytes) *part_bytes = P.gated ? (uint32_t)P.part : 0u;
    return (int)P.nsl;
}
extern "C" int trc_get_devices(int *devs, int cap)
{
    const std::vector<int> v = devs_get();
    for (int i = 0; i < (int)v.size() && i < cap; i++) devs[i] = v[i];
    return (int)v.size();
}

// ---- host-pointer encode/decode shared by every reference-signature export --------------------
// chunk_override / outcap != 0: the trc_encode_host form -- explicit chunk size, and the container is returned whatever its
// size (no folding into "== inlen means raw"); out holds outcap bytes
static size_t host_encode(int codec, const unsigned char *in, size_t inlen, unsigned char *out,
                          const cdf_t *cdf, int cdfnum, uint32_t chunk_override = 0, size_t outcap = 0)
{
    if (inlen == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fail(TRC_E_NODEV, "no HIP device: libturborc_hip has no CPU coding path"); return 0; }
    uint32_t chunk = chunk_override ? chunk_override : trc_get_chunk();
    if (!chunk) chunk = trc_auto_chunk_codec(codec, inlen);
    if (!chunk_ok(chunk)) { fail(TRC_E_ARG, "chunk %u: must be a multiple of 64 in [%u,%u]", chunk, TRC_CHUNK_MIN, TRC_CHUNK_MAX); return 0; }
    const TrcCodec &r = codec_row(codec);
    if (chunk > r.chunk_max) chunk = r.chunk_max;
    if (chunk < r.floor && !chunk_override) chunk = r.floor;    // also under TRC_CHUNK / trc_set_chunk: see trc_auto_chunk_codec
    HostJob J;
    J.codec = codec; J.chunk = chunk; J.in = in; J.out = out; J.n = inlen; J.cdf = cdf;
    J.nchunks = (inlen + chunk - 1) / chunk; J.dir = 4 * J.nchunks;
    if (outcap && outcap < J.hdrsz + J.dir + inlen) { fail(TRC_E_ARG, "encode_host: out holds %zu bytes, the container may need %zu", outcap, J.hdrsz + J.dir + inlen); return 0; }
    if (r.cdf) {
        if (cdfnum <= 0) cdfnum = host_cdfnum(cdf);
        if (cdfnum <= 0 || cdfnum > 256) { fail(TRC_E_CDF, "bad CDF (need cdf[0]=0 < ... < cdf[cdfnum]=32768)"); return 0; }
    } else if (r.ss) {
        if (cdf || !ss_prm_ok((unsigned)cdfnum)) { fail(TRC_E_ARG, "codec %d takes no CDF and cdfnum = TRC_SS_PRM(prm0, prm1) with both in 1..15 (got 0x%x)", codec, (unsigned)cdfnum); return 0; }
        J.prm = (unsigned)cdfnum; cdfnum = 0;
    } else cdfnum = 0;
    J.cdfnum = cdfnum;
    J.lim = outcap ? (size_t)-1 : inlen > J.hdrsz + J.dir ? inlen - J.hdrsz - J.dir : 0;      // payload bytes above which the call returns raw
    // page-locked caller buffers are read / written by DMA directly (no staging copy on that side)
    J.in_direct = host_is_pinned(in, inlen); J.out_direct = host_is_pinned(out, outcap ? outcap : inlen);
    const std::vector<int> devs = devs_get();
    const int nshard = devs.empty() ? 1 : (int)devs.size();
    shard_plan(J.nchunks, nshard, J.shard);
    J.total.assign((size_t)nshard, -1);
    static std::atomic<bool> gates_broken{false};
    J.no_gates = gates_broken;
    if (!run_shards(J, devs, false)) {
        if (!J.gate_timeout) { fail(TRC_E_HIP, "host encode: %s", J.err.c_str()); return 0; }
        // The arrival gates do not work in this process (something the link needs waits behind a waiting kernel): say so once, stop
        // using them, and code this call again through the slice pipeline -- nothing has been returned to the caller yet.
        fprintf(stderr, "turborc_hip: %s; host-pointer encodes of this process go back to the slice pipeline\n", J.err.c_str());
        gates_broken = true;
        J.no_gates = true; J.failed = false; J.gate_timeout = false; J.raw = false; J.err.clear();
        J.total.assign((size_t)nshard, -1);
        if (!run_shards(J, devs, false)) { fail(TRC_E_HIP, "host encode: %s", J.err.c_str()); return 0; }
    }
    if (J.raw) { memcpy(out, in, inlen); return inlen; }                    // reference convention: == inlen => raw
    size_t ppos = 0;
    for (int s = 0; s < nshard; s++) ppos += (size_t)J.total[s];
    trc_container_hdr h;
    memset(&h, 0, sizeof h);
    h.magic = TRC_MAGIC; h.codec = (uint8_t)codec; h.version = 1; h.cdfnum = (uint16_t)(cdfnum ? (unsigned)cdfnum : J.prm);
    h.chunk = chunk; h.nchunks = (uint32_t)J.nchunks; h.n = inlen; h.payload = ppos;
    memcpy(out, &h, J.hdrsz);
    return J.hdrsz + J.dir + ppos;
}

static size_t host_decode(int codec, const unsigned char *in, size_t outlen, unsigned char *out,
                          const cdf_t *cdf, int cdfnum)
{
    if (outlen == 0) return 0;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { fail(TRC_E_NODEV, "no HIP device: libturborc_hip has no CPU coding path"); return 0; }
    trc_container_hdr h;
    memcpy(&h, in, sizeof h);
    if (h.magic != TRC_MAGIC || h.version != 1 || h.codec != codec || h.n != outlen ||
        !chunk_ok(h.chunk) || h.nchunks != (outlen + h.chunk - 1) / h.chunk || h.payload > outlen) {
        fail(TRC_E_ARG, "not a TRC1 container for codec %d / length %zu (raw streams must be memcpy'd by the caller)", codec, outlen);
        return 0;
    }
    HostJob J;
    J.codec = codec; J.chunk = h.chunk; J.in = in; J.out = out; J.n = outlen; J.cdf = cdf;
    J.nchunks = h.nchunks; J.dir = 4 * J.nchunks;
    // The prototype carries no input length, so this is a SELF-CONSISTENCY test of the container, not a bound on the caller's
    // buffer: the length passed below is the one the header itself states.  It rejects truncated or inconsistent
    // directories; a forged header can still make this function read up to outlen + 4 * nchunks + 32 bytes from `in`.
    // Callers holding untrusted input must call trc_container_check(buf, REAL_LENGTH, ...) themselves first, as
    // harness/trcfile.c does.
    if (trc_container_check(in, J.hdrsz + J.dir + (size_t)h.payload, codec, outlen)) return 0;
    if (codec_row(codec).cdf) {
        if (cdfnum <= 0) cdfnum = host_cdfnum(cdf);
        if (cdfnum <= 0 || cdfnum > 256) { fail(TRC_E_CDF, "bad CDF"); return 0; }
    } else if (codec_row(codec).ss) {
        // the header's parameters (validated by trc_container_check above); a caller that states its own must state the same
        if (cdfnum && (unsigned)cdfnum != h.cdfnum) { fail(TRC_E_ARG, "codec %d: the container was coded with parameters 0x%x, the caller states 0x%x", codec, h.cdfnum, (unsigned)cdfnum); return 0; }
        J.prm = h.cdfnum; cdfnum = 0;
    } else cdfnum = 0;
    J.cdfnum = cdfnum;
    // payload offset of every group of 64 chunks, from the directory (the decoders clamp an entry above the chunk length to "raw")
    const size_t ngroups = (J.nchunks + 63) / 64;
    J.gcum.assign(ngroups + 1, 0);
    {
        uint64_t sum = 0;
        for (size_t k = 0; k < J.nchunks; k++) {
            if ((k & 63) == 0) J.gcum[k >> 6] = sum;
            uint32_t l; memcpy(&l, in + J.hdrsz + 4 * k, 4);
            const size_t len = (k + 1 == J.nchunks) ? outlen - k * (size_t)h.chunk : h.chunk;
            sum += l < len ? l : len;
        }
        J.gcum[ngroups] = sum;
    }
    J.in_direct = host_is_pinned(in, J.hdrsz + J.dir + (size_t)h.payload); J.out_direct = host_is_pinned(out, outlen);
    const std::vector<int> devs = devs_get();
    const int nshard = devs.empty() ? 1 : (int)devs.size();
    shard_plan(J.nchunks, nshard, J.shard);
    if (!run_shards(J, devs, true)) { fail(TRC_E_HIP, "host decode: %s", J.err.c_str()); return 0; }
    return outlen;
}
