// What the host drivers share: the expectation macro, the launch bookkeeping against hip_stub.cpp, the check of the
// profile names and the closing line.  TEST INFRASTRUCTURE ONLY; every driver is one translation unit with its own main.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string_view>
#include <vector>

#include "../../include/periodhip.h"

extern "C" void stub_reset_launches();
extern "C" int stub_launches(int* block, long long* lds, int cap);

static int fails = 0;
#define EXPECT(call, want)                                                              \
  do {                                                                                  \
    const int rc_ = (call);                                                             \
    if (rc_ != (want)) {                                                                \
      std::printf("FAIL %s:%d %s -> %d (%s), want %d\n", __FILE__, __LINE__, #call, rc_, ph_last_error(), (want)); \
      ++fails;                                                                          \
    }                                                                                   \
  } while (0)

// the profile name every accepted launch must have, in launch order
static std::vector<const char*> expect_names;

// a launch the driver has checked against its plan itself
[[maybe_unused]] static void launched(const char* name) { expect_names.push_back(name); }

// one launch of 256 threads without LDS since the last reset, to be found in the profile as `name`
[[maybe_unused]] static void one_launch(const char* name, int line) {
  int block[4];
  long long l[4];
  const int n = stub_launches(block, l, 4);
  if (n != 1 || block[0] != 256 || l[0] != 0) {
    std::printf("FAIL line %d: %d launches, block %d, lds %lld\n", line, n, n ? block[0] : -1, n ? l[0] : -1LL);
    ++fails;
  }
  launched(name);
  stub_reset_launches();
}

[[maybe_unused]] static void no_launch(int line) {
  int block[4];
  long long l[4];
  if (stub_launches(block, l, 4) != 0) {
    std::printf("FAIL line %d: a refused call launched a kernel\n", line);
    ++fails;
  }
  stub_reset_launches();
}

// the message of a refusal names what was refused
[[maybe_unused]] static void said(const char* word, int line) {
  const char* msg = ph_last_error();
  if (!msg || std::string_view(msg).find(word) == std::string_view::npos) {
    std::printf("FAIL line %d: message '%s' does not name %s\n", line, msg ? msg : "(null)", word);
    ++fails;
  }
}

// The `cntp` entries ph_profile_read reported (the profile keeps the first 256 launches).  With `only`, every entry
// has that name; without, the entries are the recorded launches, one each, by name.
[[maybe_unused]] static void check_profile(ph_ctx* c, int cntp, const char* only = nullptr) {
  const int want = only ? cntp : (int)(expect_names.size() < 256 ? expect_names.size() : 256);
  if (cntp != want) {
    std::printf("FAIL %d profile entries for %zu launches\n", cntp, expect_names.size());
    ++fails;
  }
  for (int i = 0; i < cntp && i < (only ? 256 : want); ++i) {
    const char* nm = ph_profile_name(c, i);
    const char* exp = only ? only : expect_names[i];
    if (!nm || std::string_view(nm) != exp) {
      std::printf("FAIL profile entry %d is %s, want %s\n", i, nm ? nm : "(null)", exp);
      ++fails;
      break;
    }
  }
}

// the closing line ("host sanitizer driver <tag> ok") and main's return value
static int finish(const char* tag) {
  if (fails) {
    std::printf("host sanitizer driver (%s): %d unexpected results\n", tag, fails);
    return 1;
  }
  std::printf("host sanitizer driver%s%s ok\n", *tag ? " " : "", tag);
  return 0;
}
