"""Source rule behind csrc/device_memory.h: a Context's device memory has one owner, so under csrc the tokens `hipMalloc(` and `hipFree(` occur only
in device_memory.h (the owner), capi.hip (memory that is the caller's: mkhe_buf_alloc and the context-less destroy path) and the handle-pool /
shared-allocator functions of engine.hip named below, with exactly these counts.  A feature that allocates on its own fails this test."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mkhe-kklss_amd", "csrc")
TOKENS = ("hipMalloc(", "hipFree(")
WHOLE_FILES = ("device_memory.h", "capi.hip")
# function of engine.hip -> (hipMalloc(, hipFree() occurrences in its body
ENGINE_FUNCS = {
    "static void* dev_alloc_bytes(size_t bytes)": (3, 0),          # the shared allocation function: one attempt, one more after the pools are trimmed, its message
    "static size_t trim_device_pools()": (0, 1),                    # every free list of the device back to the driver
    "void Context::pool_free(": (0, 2),                             # eviction over the bound; a buffer the budget has no room for
    "void Context::release_all() noexcept": (0, 1),                 # drains this context's handle pool (pool_take_all)
}


def _body(src, head):
    """the text of the function whose definition starts with `head`: from its opening brace to the matching one"""
    opens = [m.end() - 1 for m in re.finditer(re.escape(head) + r"[^;{]*\{", src)]          # (a declaration ends in ';' first)
    assert len(opens) == 1, (head, len(opens))
    depth, i, j = 0, opens[0], opens[0]
    while True:
        depth += {"{": 1, "}": -1}.get(src[j], 0)
        if depth == 0:
            return i, j + 1
        j += 1


def test_device_allocations_only_in_the_owner_the_pool_and_the_c_abi():
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".h", ".hip")) or name in WHOLE_FILES:
            continue
        src = open(os.path.join(CSRC, name)).read()
        if name == "engine.hip":
            for head, want in ENGINE_FUNCS.items():
                i, j = _body(src, head)
                got = tuple(src[i:j].count(t) for t in TOKENS)
                assert got == want, (head, got, want)
                src = src[:i] + " " * (j - i) + src[j:]
        n = sum(src.count(t) for t in TOKENS)
        if n:
            found[name] = n
    assert not found, "hipMalloc( / hipFree( outside the owner, the handle pool and the C ABI: %r" % found
    for name in WHOLE_FILES:
        assert any(t in open(os.path.join(CSRC, name)).read() for t in TOKENS), name
