// lsn_rates.h - the one table of samples per OFDM symbol (sampling mode LSN_RATES_3GPP / LSN_RATES_SRSRAN), read by Engine::buildTables and cell_search
#pragma once
#include <cstdint>

namespace lsn {
uint32_t symbol_size(uint32_t nof_prb, int rates);  // lsn_tables.cc; 0 = no such bandwidth or mode
}  // namespace lsn
