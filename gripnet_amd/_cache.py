"""What was derived from a caller's tensor, kept while the same unmodified tensor keeps coming."""
import threading
import weakref

MISS = object()             # what `get` returns when nothing matches (None is a value: "not sorted", "no plan for this list")


class VersionedCache:
    """Derived data of the last `depth` key objects, most recently used first.  An entry matches when its key object IS
    the one asked about (through a weak reference: a caller that drops its tensor takes the derived data with it, and a
    new object at a freed one's `id` never matches), the `_version` recorded at `put` is the object's current one (no
    in-place write since) and `extra` compares equal.  A value must not refer to its own key.  The lock is held for the
    look-up and the insertion only: the caller builds a value (which may synchronise the stream) outside it, and two
    threads that miss on one key both build (autograd runs a device's backward on its own thread)."""

    def __init__(self, depth: int):
        self.depth, self._entries, self._lock = depth, [], threading.Lock()

    def get(self, obj, *extra):
        ver = getattr(obj, "_version", None)
        with self._lock:
            hit, rest = None, []
            for e in self._entries:
                key = e[0]()
                if key is obj and e[1] == ver and e[2] == extra:
                    hit = e
                elif key is not None:
                    rest.append(e)
            self._entries = rest if hit is None else [hit] + rest
        return MISS if hit is None else hit[3]

    def put(self, obj, value, *extra):
        """Remember `value` for `obj` as it is now, in place of what was kept for (obj, extra); returns `value`.  An object
        without a `_version` to watch, or one that cannot be weakly referenced (a Python list), is not kept."""
        try:
            entry = (weakref.ref(obj), obj._version, extra, value)
        except (AttributeError, TypeError):
            return value
        with self._lock:
            rest = [e for e in self._entries if e[0]() is not None and not (e[0]() is obj and e[2] == extra)]
            self._entries = ([entry] + rest)[:self.depth]
        return value

    def clear(self):
        with self._lock:
            self._entries = []
