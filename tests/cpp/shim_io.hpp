// tests/cpp/shim_io.hpp -- what the shim test programs of this directory share: reading the input files, device buffers, reading a result
// back into a file, and the scaffolding of a `<program> <dir>` main.  A program on top of it is its Params struct, its context set-up, its
// calls and its output names.  Header-only and all inline: a program that leaves one of these unused still compiles clean under -Wall.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include "RendererInstance.hpp"

namespace shim_io {

inline std::vector<char> read_file(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) throw std::runtime_error("cannot read " + path);
  return {std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>()};
}

// <dir>/params.bin as the program's own Params struct; the file holds exactly that struct
template <class Params>
Params read_params(const std::string& dir) {
  const std::vector<char> raw = read_file(dir + "/params.bin");
  if (raw.size() != sizeof(Params)) throw std::runtime_error("params.bin has the wrong size");
  Params p;
  std::memcpy(&p, raw.data(), sizeof p);
  return p;
}

constexpr int no_fill = -1;

// `bytes` of device memory: first every byte set to `fill` unless that is no_fill, then the file at `path`, whose size must be `bytes`
// exactly, unless the path is empty.  The compared outputs depend on the fill, so it has no default: each call site states its own.
inline ox::amd::Buffer device_buffer(size_t bytes, int fill, const std::string& path = "") {
  void* dev = nullptr;
  if (hipMalloc(&dev, bytes) != hipSuccess || (fill != no_fill && hipMemset(dev, fill, bytes) != hipSuccess)) throw std::runtime_error("hipMalloc failed");
  if (!path.empty()) {
    const std::vector<char> host = read_file(path);
    if (host.size() != bytes || hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("upload failed: " + path);
  }
  return ox::amd::Buffer{dev, bytes};
}

// waits for everything the device was given, the passes' stream included, so a failed launch is reported here and never read back as
// stale bytes; then copies `bytes` at `dptr` into the file at `path`
inline void write_out(const std::string& path, const void* dptr, size_t bytes) {
  std::vector<char> host(bytes);
  if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("read back failed");
  std::ofstream(path, std::ios::binary).write(host.data(), (std::streamsize)host.size());
}

inline void write_out(const std::string& path, const ox::amd::Buffer& b) { write_out(path, b.dptr, b.bytes); }

// main of `<name> <dir>`: status 2 and the usage line without the one argument; otherwise body(dir), status 0, or status 1 with the
// exception's message on stderr
template <class Body>
int run(int argc, char** argv, const char* name, Body body) {
  if (argc != 2) {
    std::printf("usage: %s <dir>\n", name);
    return 2;
  }
  try {
    body(std::string(argv[1]));
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

}  // namespace shim_io
