// symbol_run.hpp -- symbol survey, host side only: what rx.cpp (the context whose edge list the survey reads) and
// symbols.cpp share beyond pulse_run.hpp's view of the last run.  No device code: the kernels' side is symbols.hpp.
#pragma once

#include "pulse_run.hpp"

namespace ookd {

struct SymbolCtx;                       // the survey's buffers, made by the first ookd_rx_symbol_survey
void symbol_ctx_free(SymbolCtx *p);     // (the caller has made the context's device current)

}  // namespace ookd

ookd::SymbolCtx **ookd_rx_symbol_ctx(ookd_rx *rx);
