// The ABI version the library was built with: the header's own number (pdgn_amd/_lib.py compares it at load).
#include "../../include/pdgn_hip.h"

extern "C" int pdgn_abi_version(void) { return PDGN_ABI_VERSION; }
