// hip_emu.cpp -- fiber scheduler behind hip_emu.hpp (CPU test infrastructure only).
#include "hip_emu.hpp"

#include <algorithm>
#include <deque>
#include <limits>
#include <map>
#include <string>
#include <vector>

namespace emu {

dim3 g_block, g_bdim, g_gdim;
Lane *g_cur = nullptr;
bool g_late = false;

namespace {

enum State { RUNNABLE, WAIT_WAVE, WAIT_BLOCK, DONE };

struct Access {
    int site, occ;
    uintptr_t addr;
    bool write;
};

// one lane's share of a vector-memory instruction, as the lane issued it (late mode)
struct VEvent {
    const char *file;
    int line;
    float *dst;                      // LDS-DMA: the wave-uniform destination; nullptr: a load or a store
    int off, ndw;
    float data[4];
    bool visible;
};

struct Fiber {
    Lane lane;
    void *sp = nullptr;
    char *stack = nullptr;
    State state = RUNNABLE;
    int index = 0;
    int xparity = 0;                 // alternates the exchange buffer (one rendez-vous per collective)
    std::vector<Access> acc;
    std::map<int, int> occ;
    std::vector<VEvent> vlog;        // vector-memory instructions issued since the wave's last rendez-vous
    int bar_kind = BAR_SYNC, bar_keep = 0, bar_line = 0;
    const char *bar_file = nullptr;
    int site_line = 0;
    const char *site_file = nullptr;
    bool wait_all = false;
};

// one wave instruction in flight
struct LaneWrite { float *dst; int ndw; float data[4]; };
struct VEntry {
    const char *file;
    int line;
    bool dma, visible;
    bool unordered;                  // not one instruction: what the lanes of a wave issued in no order the source determines
    int lane_a, lane_b;              // ... the two lanes that disagreed (file / line: what lane_a issued and lane_b did not)
    std::vector<LaneWrite> writes;
};
struct SiteStat { unsigned long long runs = 0, unlanded = 0; int max_keep = -1, max_keep_unlanded = -1; };
struct VStats {
    unsigned long long dma_issued = 0, retired_counted = 0;
    std::map<std::string, SiteStat> sites;
};

constexpr size_t kStack = 256 * 1024;
std::vector<Fiber> fibers;
std::vector<uint64_t> xbuf;          // [wave][parity][64]
std::vector<unsigned char> xwide;    // [wave][parity][64][32]
void *sched_sp = nullptr;
Fiber *cur_fiber = nullptr;
const std::function<void()> *cur_body = nullptr;
Stats g_stats = {};
void *lds_base = nullptr;
size_t lds_bytes = 0;
bool lds_trace = false;
bool reversed = false;
int keep_plus = 0;
std::vector<std::deque<VEntry>> vqueue;      // [wave]
VStats g_vstats;

extern "C" void emu_switch(void **save_sp, void *load_sp);
asm(R"(
.text
.globl emu_switch
.type emu_switch,@function
emu_switch:
    pushq %rbp
    pushq %rbx
    pushq %r12
    pushq %r13
    pushq %r14
    pushq %r15
    movq %rsp, (%rdi)
    movq %rsi, %rsp
    popq %r15
    popq %r14
    popq %r13
    popq %r12
    popq %rbx
    popq %rbp
    ret
)");

void yield_to_scheduler() { emu_switch(&cur_fiber->sp, sched_sp); }

void fiber_entry() {
    (*cur_body)();
    cur_fiber->state = DONE;
    yield_to_scheduler();
    std::fprintf(stderr, "emu: resumed a finished fiber\n");
    std::abort();
}

void prepare(Fiber &f) {
    if (!f.stack) f.stack = static_cast<char *>(std::malloc(kStack));
    uintptr_t top = (reinterpret_cast<uintptr_t>(f.stack) + kStack) & ~uintptr_t(15);
    void **s = reinterpret_cast<void **>(top);
    s[-1] = nullptr;                                   // fake return address of fiber_entry
    s[-2] = reinterpret_cast<void *>(&fiber_entry);    // popped by emu_switch's ret
    for (int i = 3; i <= 8; ++i) s[-i] = nullptr;      // rbp rbx r12 r13 r14 r15
    f.sp = &s[-8];
    f.state = RUNNABLE;
    f.xparity = 0;
    f.acc.clear();
    f.occ.clear();
    f.vlog.clear();
    f.site_line = 0;
    f.site_file = nullptr;
    f.wait_all = false;
}

std::string site_name(const char *file, int line) {
    const char *base = file ? std::strrchr(file, '/') : nullptr;
    return std::string(base ? base + 1 : (file ? file : "?")) + ":" + std::to_string(line);
}

bool same_instr(const VEvent &a, const VEvent &b) { return a.line == b.line && a.file == b.file && a.dst == b.dst; }

// Lanes are separate fibers: the instructions they issued since the wave's last rendez-vous are grouped into wave instructions
// here.  The order is the longest lane's; every other lane's sequence must be a subsequence of it (instruction = source line +,
// for a DMA, the wave-uniform LDS destination).  A wave whose lanes disagree -- two lanes that each issued something the other
// did not, the two sides of a divergent branch -- has no order, and no count, that the source determines.  What it issued is
// queued as ONE unordered entry: harmless where a wait retires it whole (the stores of an epilogue), fatal where a counted
// barrier would have to count it (retire_at_barrier) -- the emulator stops rather than guess.
void merge_wave(int w, int nthreads) {
    int lo = w * 64, hi = std::min(nthreads, lo + 64), longest = -1;
    for (int t = lo; t < hi; ++t)
        if (!fibers[t].vlog.empty() && (longest < 0 || fibers[t].vlog.size() > fibers[longest].vlog.size())) longest = t;
    if (longest < 0) return;
    const std::vector<VEvent> ref = fibers[longest].vlog;
    std::vector<VEntry> merged(ref.size());
    for (size_t i = 0; i < ref.size(); ++i)
        merged[i] = VEntry{ref[i].file, ref[i].line, ref[i].dst != nullptr, ref[i].visible, false, 0, 0, {}};
    VEntry group{nullptr, 0, false, false, false, 0, 0, {}};
    for (int t = lo; t < hi && !group.unordered; ++t) {
        size_t at = 0;
        for (const VEvent &e : fibers[t].vlog) {
            while (at < ref.size() && !same_instr(ref[at], e)) ++at;
            if (at == ref.size()) {
                group = VEntry{e.file, e.line, false, false, true, t - lo, longest - lo, {}};
                break;
            }
            if (e.dst) {
                LaneWrite lw{e.dst + e.off, e.ndw, {e.data[0], e.data[1], e.data[2], e.data[3]}};
                merged[at].writes.push_back(lw);
            }
            ++at;
        }
    }
    if (group.unordered) {
        merged.clear();
        for (int t = lo; t < hi; ++t)
            for (const VEvent &e : fibers[t].vlog)
                if (e.dst) {
                    LaneWrite lw{e.dst + e.off, e.ndw, {e.data[0], e.data[1], e.data[2], e.data[3]}};
                    group.writes.push_back(lw);
                    group.dma = true;
                    group.visible |= e.visible;
                }
        merged.push_back(group);
    }
    for (int t = lo; t < hi; ++t) fibers[t].vlog.clear();
    for (VEntry &m : merged) {
        if (m.dma && !m.unordered) g_vstats.dma_issued++;
        vqueue[w].push_back(std::move(m));
    }
}

void retire_oldest(int w) {
    VEntry &e = vqueue[w].front();
    for (const LaneWrite &lw : e.writes) std::memcpy(lw.dst, lw.data, size_t(lw.ndw) * 4);
    vqueue[w].pop_front();
}

[[noreturn]] void cannot_count(int w, const VEntry &e, const char *what, const char *file, int line) {
    std::fprintf(stderr, "emu: block (%u,%u,%u) wave %d: %s %s has to count vector-memory instructions that have no single order: "
                 "lane %d issued %s where lane %d, with the longest sequence, did not\n", g_block.x, g_block.y, g_block.z, w, what,
                 site_name(file, line).c_str(), e.lane_a, site_name(e.file, e.line).c_str(), e.lane_b);
    std::abort();
}

int unlanded(int w) {
    int n = 0;
    for (const VEntry &e : vqueue[w]) n += e.dma;
    return n;
}

// the block barrier is about to be released: every wave waits for what its barrier makes it wait for
void retire_at_barrier(int w, int nthreads) {
    int lo = w * 64, hi = std::min(nthreads, lo + 64);
    const Fiber *first = nullptr;
    for (int t = lo; t < hi; ++t) {
        const Fiber &f = fibers[t];
        if (f.state != WAIT_BLOCK) continue;
        if (!first) first = &f;
        else if (f.bar_kind != first->bar_kind || f.bar_keep != first->bar_keep || f.bar_line != first->bar_line) {
            std::fprintf(stderr, "emu: block (%u,%u,%u) wave %d: lanes %d and %d meet in different barriers (%s keep %d, %s keep %d)\n",
                         g_block.x, g_block.y, g_block.z, w, first->index - lo, t - lo,
                         site_name(first->bar_file, first->bar_line).c_str(), first->bar_keep,
                         site_name(f.bar_file, f.bar_line).c_str(), f.bar_keep);
            std::abort();
        }
    }
    if (!first) return;
    std::deque<VEntry> &q = vqueue[w];
    if (first->bar_kind == BAR_SYNC) {
        int youngest = -1;
        for (size_t i = 0; i < q.size(); ++i)
            if (q[i].dma && q[i].visible) youngest = int(i);
        // (an unordered entry that holds a visible fill and is the last to go: what else of it the barrier waits for is unknown)
        if (youngest >= 0 && q[youngest].unordered) cannot_count(w, q[youngest], "__syncthreads() at", first->bar_file, first->bar_line);
        for (int i = 0; i <= youngest; ++i) retire_oldest(w);
    } else if (first->bar_kind == BAR_KEEP) {
        SiteStat &st = g_vstats.sites[site_name(first->bar_file, first->bar_line)];
        const int keep = std::max(0, first->bar_keep), pending = unlanded(w);
        st.runs++;
        st.max_keep = std::max(st.max_keep, keep);
        if (pending) {
            st.unlanded++;
            st.max_keep_unlanded = std::max(st.max_keep_unlanded, keep);
        }
        for (int i = 0; i < keep + keep_plus && i < int(q.size()); ++i)            // the entries the count is counted in
            if (q[q.size() - 1 - i].unordered)
                cannot_count(w, q[q.size() - 1 - i], "the counted barrier at", first->bar_file, first->bar_line);
        while (int(q.size()) > keep + keep_plus) {
            if (q.front().dma) g_vstats.retired_counted++;
            retire_oldest(w);
        }
    }
}

void analyse_lds(int nthreads) {
    if (!lds_trace) return;
    int nwaves = (nthreads + 63) / 64;
    for (int w = 0; w < nwaves; ++w) {
        std::map<std::pair<int, int>, std::vector<std::pair<int, uintptr_t>>> groups[2];
        for (int l = 0; l < 64 && w * 64 + l < nthreads; ++l)
            for (const Access &a : fibers[w * 64 + l].acc)
                groups[a.write][{a.site, a.occ}].push_back({l, a.addr});
        for (int wr = 0; wr < 2; ++wr)
            for (auto &kv : groups[wr]) {
                unsigned cycles = 0;
                for (int half = 0; half < 2; ++half) {
                    std::map<unsigned, std::vector<uintptr_t>> banks;
                    for (auto &la : kv.second)
                        if (la.first / 32 == half) {
                            auto &v = banks[(la.second / 4) % 32];
                            if (std::find(v.begin(), v.end(), la.second) == v.end()) v.push_back(la.second);
                        }
                    unsigned worst = 0;
                    for (auto &b : banks) worst = std::max<unsigned>(worst, b.second.size());
                    cycles += worst;
                }
                if (wr) { g_stats.lds_write_instr++; g_stats.lds_write_cycles += cycles; }
                else    { g_stats.lds_read_instr++;  g_stats.lds_read_cycles += cycles; }
            }
    }
}

void run_block(int nthreads) {
    int nwaves = (nthreads + 63) / 64;
    xbuf.assign(size_t(nwaves) * 2 * 64, 0);
    xwide.assign(size_t(nwaves) * 2 * 64 * 32, 0);
    for (int t = 0; t < nthreads; ++t) prepare(fibers[t]);
    vqueue.assign(nwaves, {});
    for (;;) {
        bool progressed = false, all_done = true;
        for (int i = 0; i < nthreads; ++i) {
            Fiber &f = fibers[reversed ? nthreads - 1 - i : i];
            if (f.state == DONE) continue;
            all_done = false;
            if (f.state != RUNNABLE) continue;
            cur_fiber = &f;
            g_cur = &f.lane;
            emu_switch(&sched_sp, f.sp);
            progressed = true;
        }
        if (all_done) break;
        // release wave rendez-vous
        for (int w = 0; w < nwaves; ++w) {
            int lo = w * 64, hi = std::min(nthreads, lo + 64), waiting = 0, alive = 0;
            for (int t = lo; t < hi; ++t) {
                if (fibers[t].state != DONE) ++alive;
                if (fibers[t].state == WAIT_WAVE) ++waiting;
            }
            if (alive && waiting == alive) {
                bool wait_all = false;
                for (int t = lo; t < hi; ++t)
                    if (fibers[t].state == WAIT_WAVE) {
                        fibers[t].state = RUNNABLE;
                        wait_all |= fibers[t].wait_all;
                        fibers[t].wait_all = false;
                    }
                if (g_late) {
                    merge_wave(w, nthreads);
                    while (wait_all && !vqueue[w].empty()) retire_oldest(w);
                }
                progressed = true;
            }
        }
        // release block barrier
        int waiting = 0, alive = 0;
        for (int t = 0; t < nthreads; ++t) {
            if (fibers[t].state != DONE) ++alive;
            if (fibers[t].state == WAIT_BLOCK) ++waiting;
        }
        if (alive && waiting == alive) {
            if (g_late)
                for (int w = 0; w < nwaves; ++w) {
                    merge_wave(w, nthreads);
                    retire_at_barrier(w, nthreads);
                }
            for (int t = 0; t < nthreads; ++t)
                if (fibers[t].state == WAIT_BLOCK) fibers[t].state = RUNNABLE;
            progressed = true;
        }
        if (!progressed) {
            std::fprintf(stderr, "emu: deadlock in block (%u,%u,%u): divergent barrier or collective\n",
                         g_block.x, g_block.y, g_block.z);
            std::abort();
        }
    }
    if (g_late)                                            // the end of the kernel: everything lands
        for (int w = 0; w < nwaves; ++w) {
            merge_wave(w, nthreads);
            while (!vqueue[w].empty()) retire_oldest(w);
        }
    analyse_lds(nthreads);
}

}  // namespace

void launch(dim3 grid, dim3 block, const std::function<void()> &body) {
    const char *env = std::getenv("CCA_EMU_LDS");
    lds_trace = env && env[0] == '1';
    auto on = [](const char *name) { const char *v = std::getenv(name); return v && v[0] == '1'; };
    g_late = on("CCA_EMU_LATE_DMA");
    reversed = on("CCA_EMU_REVERSE");
    keep_plus = on("CCA_EMU_KEEP_PLUS") ? 1 : 0;
    g_gdim = grid;
    g_bdim = block;
    int nthreads = int(block.x * block.y * block.z);
    if (int(fibers.size()) < nthreads) fibers.resize(nthreads);
    for (int t = 0; t < nthreads; ++t) {
        fibers[t].index = t;
        fibers[t].lane.tid = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
    }
    cur_body = &body;
    g_stats.launches++;
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned y = 0; y < grid.y; ++y)
            for (unsigned x = 0; x < grid.x; ++x) {
                g_block = dim3(x, y, z);
                lds_base = nullptr;
                lds_bytes = 0;
                run_block(nthreads);
            }
    cur_body = nullptr;
}

void block_barrier(int kind, int keep, int line, const char *file) {
    Fiber &f = *cur_fiber;
    f.bar_kind = kind;
    f.bar_keep = keep;
    f.bar_line = f.site_file ? f.site_line : line;
    f.bar_file = f.site_file ? f.site_file : file;
    f.site_file = nullptr;
    f.state = WAIT_BLOCK;
    yield_to_scheduler();
}

void set_barrier_site(int line, const char *file) {
    cur_fiber->site_line = line;
    cur_fiber->site_file = file;
}

void vmem_note(int line, const char *file) {
    if (g_late) cur_fiber->vlog.push_back(VEvent{file, line, nullptr, 0, 0, {0, 0, 0, 0}, false});
}

void vmem_dma(int line, const char *file, float *dst_wave_base, int lane_dword_off, const float *data, int ndw, bool compiler_visible) {
    if (!g_late) {
        std::memcpy(dst_wave_base + lane_dword_off, data, size_t(ndw) * 4);
        return;
    }
    VEvent e{file, line, dst_wave_base, lane_dword_off, ndw, {0, 0, 0, 0}, compiler_visible};
    std::memcpy(e.data, data, size_t(ndw) * 4);
    cur_fiber->vlog.push_back(e);
}

void vmem_wait_all() {
    if (!g_late) return;
    Fiber &f = *cur_fiber;
    f.wait_all = true;
    f.state = WAIT_WAVE;
    yield_to_scheduler();
}

int lane_id() { return cur_fiber->index & 63; }

const uint64_t *wave_exchange(uint64_t mine) {
    Fiber &f = *cur_fiber;
    int wave = f.index / 64;
    uint64_t *slots = &xbuf[(size_t(wave) * 2 + f.xparity) * 64];
    f.xparity ^= 1;
    slots[f.index & 63] = mine;
    f.state = WAIT_WAVE;
    yield_to_scheduler();
    return slots;
}

const unsigned char *wave_exchange_bytes(const void *mine, size_t nbytes) {
    Fiber &f = *cur_fiber;
    int wave = f.index / 64;
    unsigned char *slots = &xwide[(size_t(wave) * 2 + f.xparity) * 64 * 32];
    f.xparity ^= 1;
    std::memcpy(slots + size_t(f.index & 63) * 32, mine, nbytes <= 32 ? nbytes : 32);
    f.state = WAIT_WAVE;
    yield_to_scheduler();
    return slots;
}

void lds_register(void *base, size_t bytes) {
    // first caller of the block wins; it runs before any other fiber touches LDS, and the
    // kernel follows the registration with a __syncthreads().
    // (a kernel may register several __shared__ arrays: each is poisoned once per block, by its first caller)
    static void *seen[8];
    static int nseen = 0;
    if (!lds_base) nseen = 0;                                // first registration of this block
    for (int i = 0; i < nseen; ++i)
        if (seen[i] == base) return;
    if (nseen < 8) seen[nseen++] = base;
    if (!lds_base) {
        lds_base = base;
        lds_bytes = bytes;
    }
    uint32_t *p = static_cast<uint32_t *>(base);
    for (size_t i = 0; i < bytes / 4; ++i) p[i] = 0x7fc0dead;
}

static void note(const void *addr, int site, bool write) {
    if (!lds_trace) return;
    Fiber &f = *cur_fiber;
    int occ = f.occ[site * 2 + write]++;
    f.acc.push_back({site, occ, reinterpret_cast<uintptr_t>(addr), write});
}
void lds_note_read(const void *addr, int site) { note(addr, site, false); }
void lds_note_write(const void *addr, int site) { note(addr, site, true); }

Stats &stats() { return g_stats; }
static VStats &vmem_stats() { return g_vstats; }

}  // namespace emu

// emulator-only exports (not part of include/ccnet_cca.h): counters for the tests
extern "C" void cca_emu_stats(unsigned long long *out6) {
    const emu::Stats &s = emu::stats();
    out6[0] = s.lds_read_instr; out6[1] = s.lds_read_cycles; out6[2] = s.lds_write_instr;
    out6[3] = s.lds_write_cycles; out6[4] = s.mfma; out6[5] = s.launches;
}
extern "C" void cca_emu_reset_stats() { emu::stats() = emu::Stats{}; }

// the vector-memory model's counters (late mode), as text: "dma_issued N", "retired_by_counted_barriers N", then per source line
// of a counted barrier "site FILE:LINE RUNS RUNS_WITH_AN_UNLANDED_DMA MAX_KEEP MAX_KEEP_WITH_AN_UNLANDED_DMA" (-1: never).
// Returns the length of the whole text; writes at most cap - 1 characters of it and a terminator.
extern "C" size_t emu_vmem_stats(char *out, size_t cap) {
    const emu::VStats &v = emu::vmem_stats();
    std::string s = "dma_issued " + std::to_string(v.dma_issued) + "\nretired_by_counted_barriers " + std::to_string(v.retired_counted) + "\n";
    for (const auto &kv : v.sites)
        s += "site " + kv.first + " " + std::to_string(kv.second.runs) + " " + std::to_string(kv.second.unlanded) + " " +
             std::to_string(kv.second.max_keep) + " " + std::to_string(kv.second.max_keep_unlanded) + "\n";
    if (out && cap) {
        const size_t n = std::min(cap - 1, s.size());
        std::memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return s.size();
}
extern "C" void emu_vmem_reset_stats() { emu::vmem_stats() = emu::VStats{}; }
