// p2s_error.h -- the one error function of the library: formats the text that p2s_last_error() returns on this thread
// and hands `code` back, so that a refusal reads `return p2s_set_error(code, ...)`.  Defined in p2s_api.hip; plain C++,
// so that the host-only translation units (p2s_ingest.cpp, p2s_trc.cpp, ...) include it without HIP.
#ifndef P2S_ERROR_H
#define P2S_ERROR_H

int p2s_set_error(int code, const char *fmt, ...);

#endif
