#!/bin/bash
# tools/tsan_adapt.sh -- csrc/smh_adapt.h (the adaptive engine's host state and policy) under ThreadSanitizer on the CPU.
# With the mutex: no report.  Without it ("nolock"): ThreadSanitizer must report, i.e. the harness sees what the mutex guards.
# Binary and logs go to a private temporary directory (TSAN_OUT keeps them), so that users of one machine do not collide.
# The binary runs with address-space randomisation off for its own process (setarch -R): ThreadSanitizer's fixed shadow
# layout does not fit a kernel's high-entropy mmap randomisation ("FATAL: ThreadSanitizer: unexpected memory mapping").
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
T=${TSAN_OUT:-$(mktemp -d)}
[ -n "$TSAN_OUT" ] || trap 'rm -rf "$T"' EXIT
mkdir -p "$T"
NORAND=()
if command -v setarch > /dev/null && setarch "$(uname -m)" -R true 2> /dev/null; then NORAND=(setarch "$(uname -m)" -R); fi
g++ -std=c++17 -O1 -g -fsanitize=thread -I"$ROOT/cuda-aho-corasick-wu-manber_amd/csrc" "$ROOT/tools/tsan_adapt.cpp" -o "$T/tsan_adapt" -pthread
"${NORAND[@]}" "$T/tsan_adapt" 2>&1 | tee "$T/tsan_adapt.log"
if grep -q "ThreadSanitizer" "$T/tsan_adapt.log"; then echo "TSAN REPORTS with the mutex held"; exit 1; fi
if "${NORAND[@]}" "$T/tsan_adapt" nolock > "$T/tsan_adapt_nolock.log" 2>&1 && ! grep -q "ThreadSanitizer" "$T/tsan_adapt_nolock.log"; then
    echo "note: the unlocked run raised no report this time (races are timing-dependent)"
else
    echo "unlocked control run: ThreadSanitizer reports $(grep -c 'WARNING: ThreadSanitizer' "$T/tsan_adapt_nolock.log") race(s), as expected"
fi
echo "tsan: clean with the mutex"
