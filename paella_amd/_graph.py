"""The owner protocol of a captured HIP graph: what `GraphSampler`, `RequestStream` (paella_amd/sampling.py) and `GraphTrainStep` (paella_amd/training.py) share.

An owner holds ONE captured graph and the state the capture depended on besides its shapes.  Before every replay it compares that state with the present one
and, on a difference, captures again or refuses.  The capture sequence -- warm-up on a side stream, join, synchronise, take the state, capture, synchronise --
is written here once.  A leaf module: it imports torch and nothing of the package.
"""
import torch


class GraphOwner:
    """An object that owns one captured graph.  The owner brings `device`, `_state()` -- the (name, value) pairs the capture depends on besides the shapes -- and
    `_capture()`, which (re)builds whatever the graph needs and ends in `_capture_graph`; its `__init__` calls `_init_owner` before the first capture."""

    _noun = "captured graph"  # what the stale message calls the capture
    _stale_hint = ""          # the routes by which the state usually changes, for the stale message

    def _init_owner(self, on_stale):
        if on_stale not in ("recapture", "raise"):
            raise ValueError("on_stale must be 'recapture' or 'raise'")
        self.on_stale = on_stale
        self.captures = 0

    def _capture_graph(self, run, warmup=None, n_warmup=2, after_warmup=None, after_capture=None):
        """run() captured into a HIP graph on self.device -> what run() returned inside the capture; sets self.graph and self._captured_state, counts
        self.captures.  warmup (default: run) runs n_warmup times on a side stream first; after_warmup() is called once the current stream has joined the side
        stream, after_capture() when the capture has ended, each ahead of a device synchronise."""
        dev = self.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(n_warmup):  # warm-up: weights (re)loaded, workspaces sized, allocator pools populated
                (warmup or run)()
        torch.cuda.current_stream(dev).wait_stream(side)
        if after_warmup is not None:
            after_warmup()
        torch.cuda.synchronize(dev)
        state = self._state()  # AFTER the warm-up: the engines are loaded with exactly these tensors
        graph = torch.cuda.CUDAGraph()
        # thread_local: a process-group watchdog thread polling events must not invalidate the capture
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = run()
        if after_capture is not None:
            after_capture()
        torch.cuda.synchronize(dev)
        self.graph, self._captured_state = graph, state
        self.captures += 1
        return out

    def _stale(self):
        """what the capture depends on and has changed since, by name (empty: the capture is fresh)"""
        return [a[0] for a, b in zip(self._state(), self._captured_state) if a != b]

    def _refuse_recapture(self, causes):
        """the owner's veto: raise here when a stale capture must neither be replaced nor reported as merely stale (RequestStream: requests in flight)"""

    def _check_fresh(self):
        """what every replay starts with: nothing when the capture is fresh, else a new capture (on_stale="recapture") or a RuntimeError that names the causes"""
        causes = self._stale()
        if not causes:
            return
        self._refuse_recapture(causes)
        if self.on_stale == "raise":
            name = type(self).__name__
            raise RuntimeError("%s: the %s is stale -- changed since the capture: %s%s.  Build a new %s or construct it with on_stale='recapture'."
                               % (name, self._noun, ", ".join(causes), self._stale_hint and " (%s)" % self._stale_hint, name))
        self._capture()
