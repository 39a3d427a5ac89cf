// cca_emu_tu.cpp (tests/emu) -- the translation unit of the emulator build of ccnet_amd/csrc/cca_api.hip.  Test infrastructure only.
//
// barrier_dma_keep_n(expr) of cca_common.hpp dispatches to barrier_dma_keep<N>() from inside a switch, so the counted barrier's
// own line is the same for every caller.  With the helper's definition already seen, this macro charges the barrier to the line
// of the CALL instead (emu::set_barrier_site), so that the vector-memory model's per-site counters name the kernel's line.
#include <cca_common.hpp>
#define barrier_dma_keep_n(...) (emu::set_barrier_site(__LINE__, __FILE__), barrier_dma_keep_n(__VA_ARGS__))
#include "cca_api.hip"

// emulator-only export: the device id and CU count the host code sees from now on (id 0, 0 CUs: the default)
extern "C" void cca_emu_set_device(int dev, int cus) {
    cca_emu_device()[0] = dev;
    cca_emu_device()[1] = cus;
}
