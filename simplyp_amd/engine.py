"""ctypes binding of libsimplyp_hip.so (the C ABI in include/simplyp.h).

The library is built in-tree by ``__graft_entry__.build()`` into
``simplyp_amd/csrc/libsimplyp_hip.so``.  There is no CPU fallback: if the library
or a HIP device is missing, every entry point here raises.

torch is used for plumbing only: device buffers, the current HIP stream and
(in ensemble.py) ``torch.distributed``.
"""

import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB_PATH = os.environ.get('SIMPLYP_HIP_LIB') or os.path.join(CSRC, 'libsimplyp_hip.so')   # env: experiments only
INCLUDE = os.path.join(os.path.dirname(HERE), 'include')

_lib = None


class EngineError(RuntimeError):
    pass


def prototypes(text):
    """[(name, restype, argtypes)] of every ``ret simplyp_name(params);`` that header text declares, in its order, with the types
    of abi.C_SCALARS / abi.C_RETURNS.  Whatever else follows a ``simplyp_name(`` raises: nothing is skipped."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)                        # comments
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', ' ', text, flags=re.M)            # preprocessor lines and their continuations
    structs = abi.structs()
    squeeze = lambda t: re.sub(r'\s*\*', '*', ' '.join(t.split()))                    # 'const  char *' -> 'const char*'
    out = []
    for m in re.finditer(r'\b(simplyp_\w+)\s*\(', text):
        name = m.group(1)
        start = max(text.rfind(c, 0, m.start()) for c in ';{}') + 1
        ret = squeeze(text[start:m.start()])
        params = re.match(r'([^()]*)\)\s*;', text[m.end():])
        if ret not in abi.C_RETURNS or params is None:
            raise EngineError("include/simplyp.h: cannot read the declaration of %s" % name)
        argtypes = []
        for param in [squeeze(x) for x in params.group(1).split(',')] if squeeze(params.group(1)) != 'void' else []:
            pm = re.fullmatch(r'(?:const )?(\w+)(?:(\*+) ?| )\w+', param)
            base, stars = pm.groups() if pm else (None, None)
            if stars:
                argtypes.append(C.POINTER(structs[base]) if stars == '*' and base in structs else C.c_void_p)
            elif base in abi.C_SCALARS:
                argtypes.append(abi.C_SCALARS[base])
            else:
                raise EngineError("include/simplyp.h: %s: no ctypes type for the parameter '%s'" % (name, param))
        out.append((name, abi.C_RETURNS[ret], argtypes))
    return out


with open(os.path.join(INCLUDE, 'simplyp.h')) as _fh:
    PROTOTYPES = prototypes(_fh.read())
ABI_SYMBOLS = [_name for _name, _, _ in PROTOTYPES]         # every symbol include/simplyp.h declares
# include/simplyp_residuals.h: the extension header (the lag-one sums and the AR(1) log-probability), read the same way
with open(os.path.join(INCLUDE, 'simplyp_residuals.h')) as _fh:
    RESIDUALS_PROTOTYPES = prototypes(_fh.read())
RESIDUALS_SYMBOLS = [_name for _name, _, _ in RESIDUALS_PROTOTYPES]
# include/simplyp_nsga2.h: the extension header of NSGA-II's pieces (initial population, crowding, selection, offspring)
with open(os.path.join(INCLUDE, 'simplyp_nsga2.h')) as _fh:
    NSGA2_PROTOTYPES = prototypes(_fh.read())
NSGA2_SYMBOLS = [_name for _name, _, _ in NSGA2_PROTOTYPES]


def build(force=False, verbose=False):
    """Compile the HIP library for gfx950 (hipcc cross-compiles without a GPU)."""
    main = os.path.join(CSRC, 'simplyp_hip.hip')
    # everything the one translation unit can include: a header left out here would leave a stale library in use
    srcs = glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')) + glob.glob(os.path.join(INCLUDE, '*.h'))
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    # -ffp-contract=off: every fused multiply-add in the kernels is written explicitly, so the chain kernel and the
    # task-queue kernel (same source, different inlining context) round identically and stay bit-for-bit equal
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fPIC', '-shared',
           '-o', LIB_PATH, main]
    if verbose:
        cmd.insert(1, '-Rpass-analysis=kernel-resource-usage')
    subprocess.check_call(cmd)
    return LIB_PATH


def lib():
    """The loaded library; raises EngineError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineError("HIP engine library not found at %s -- build it with "
                          "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); "
                          "there is no CPU fallback" % LIB_PATH)
    # torch bundles its own HIP runtime (same SONAME as /opt/rocm's): load torch first so that this
    # library binds to the runtime that owns the process' device tensors and streams.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, restype, argtypes in PROTOTYPES + RESIDUALS_PROTOTYPES + NSGA2_PROTOTYPES:
        fn = getattr(L, name, None)
        if fn is None:
            raise EngineError("libsimplyp_hip.so lacks the declared symbol %s -- rebuild" % name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.simplyp_abi_version() != abi.ABI_VERSION:
        raise EngineError("libsimplyp_hip.so has ABI %d, the Python host expects %d -- rebuild"
                          % (L.simplyp_abi_version(), abi.ABI_VERSION))
    _lib = L
    return L


def plan(up_ptr, up_idx):
    """Routing schedule for a reach graph (host only): dict of per-reach int arrays + totals."""
    up_ptr = np.ascontiguousarray(up_ptr, dtype=np.int32)
    up_idx = np.ascontiguousarray(up_idx, dtype=np.int32)
    S = len(up_ptr) - 1
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    nl, ns = C.c_int32(), C.c_int32()
    arrs = [np.full(S, -2, dtype=np.int32) for _ in range(4)]
    dummy = np.zeros(1, dtype=np.int32)
    rc = lib().simplyp_plan(S, ip(up_ptr), ip(up_idx if up_idx.size else dummy), C.byref(nl), C.byref(ns), *[ip(a) for a in arrs])
    if rc != 0:
        raise EngineError("simplyp_plan failed (%d): %s" % (rc, lib().simplyp_last_error(None).decode()))
    return dict(n_launches=nl.value, n_slots=ns.value, launch=arrs[0], chain=arrs[1], pos=arrs[2], route_slot=arrs[3])


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


class _PinnedBlock(object):
    """Owner of one simplyp_host_alloc block; freed when the last numpy view dies."""

    def __init__(self, nbytes):
        self.ptr = lib().simplyp_host_alloc(C.c_int64(max(int(nbytes), 1)))
        if not self.ptr:
            raise EngineError("simplyp_host_alloc(%d bytes) failed (pinned host memory)" % nbytes)
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                lib().simplyp_host_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def bind_host_thread_to_gpu_numa_node(device=0):
    """Best effort: pin the calling thread (and what it allocates next: page-locked buffers are placed by first touch) to
    the CPUs of the NUMA node the GPU hangs off, so that a rank's 44 GB staging buffer and its PCIe link are on the same
    socket when 8 ranks stream at once.  Returns the node number or None (no sysfs entry, single-node machine, no
    permission): never raises."""
    try:
        import torch
        pr = torch.cuda.get_device_properties(device)
        bdf = '%04x:%02x:%02x.0' % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        with open('/sys/bus/pci/devices/%s/numa_node' % bdf) as fh:
            node = int(fh.read().strip())
        if node < 0:
            return None
        with open('/sys/devices/system/node/node%d/cpulist' % node) as fh:
            cpus = set()
            for part in fh.read().strip().split(','):
                lo, _, hi = part.partition('-')
                cpus.update(range(int(lo), int(hi or lo) + 1))
        allowed = os.sched_getaffinity(0) & cpus
        if not allowed:
            return None
        os.sched_setaffinity(0, allowed)
        return node
    except Exception:
        return None


def pinned_empty(shape, dtype=np.float64):
    """numpy array in page-locked host memory (simplyp_host_alloc = hipHostMalloc): what the marshalling code fills and
    what ``Engine.run(..., host_out=...)`` streams the output table into, so that both directions move at PCIe speed
    and asynchronously.  Needs the library and a HIP device."""
    dtype = np.dtype(dtype)
    shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    blk = _PinnedBlock(n * dtype.itemsize)
    buf = (C.c_char * max(blk.nbytes, 1)).from_address(blk.ptr)
    buf._owner = blk                                 # keeps the block alive as long as any view of it
    return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)


class Engine(object):
    """One device context.  ``run`` takes device tensors (torch) and returns device tensors."""

    def __init__(self, device=0, use_torch_stream=True):
        import torch
        self.torch = torch
        L = lib()
        if not torch.cuda.is_available() or L.simplyp_device_count() <= 0:
            raise EngineError("no HIP device visible: the SimplyP engine runs on MI355X only (no CPU fallback)")
        self.device = int(device)
        self.tdev = torch.device('cuda', self.device)
        h = C.c_void_p()
        rc = L.simplyp_ctx_create(self.device, C.byref(h))
        if rc != 0:
            raise EngineError("simplyp_ctx_create(%d) failed (%d): %s"
                              % (self.device, rc, L.simplyp_last_error(None).decode()))
        self._h = h
        self._use_torch_stream = use_torch_stream

    def close(self):
        if getattr(self, '_h', None):
            lib().simplyp_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _bind_stream(self):
        """Order the library's launches after whatever the caller has enqueued on torch's current stream.  A real torch
        stream is handed to the library and used as is.  Torch's DEFAULT stream has handle 0, which the library would read
        as "use your private stream" -- a non-blocking stream that is not ordered with the default stream at all -- so in
        that case the pending work (input casts, the caller's own kernels) is waited for here and the context keeps its one
        private stream.  The run itself is synchronous, so consumers on any stream are safe afterwards."""
        torch = self.torch
        cur = torch.cuda.current_stream(self.tdev)
        handle = cur.cuda_stream if self._use_torch_stream else 0
        if handle:
            self._check(lib().simplyp_ctx_set_stream(self._h, C.c_void_p(handle)), 'simplyp_ctx_set_stream')
        else:
            cur.synchronize()
            self._check(lib().simplyp_ctx_set_stream(self._h, None), 'simplyp_ctx_set_stream')

    def _check(self, rc, what):
        if rc != 0:
            raise EngineError("%s failed (%d): %s" % (what, rc, lib().simplyp_last_error(self._h).decode()))

    def to_device(self, a, dtype=None):
        """numpy / torch -> contiguous device tensor."""
        torch = self.torch
        if isinstance(a, torch.Tensor):
            t = a.to(self.tdev)
            if dtype is not None:
                t = t.to(dtype)
            return t.contiguous()
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:
            a = a.copy()
        t = torch.from_numpy(a)
        if dtype is not None:
            t = t.to(dtype)
        # page-locked sources (engine.pinned_empty) go up as an asynchronous DMA on torch's current stream, which the run
        # is ordered after (_bind_stream); pageable ones are staged synchronously by torch either way
        return t.to(self.tdev, non_blocking=True).contiguous()

    def run(self, forcing, doy, member_params, reach_params, up_ptr, up_idx, opts, forcing_of_member=None,
            out_reaches=None, out=None, member_rhs=None, member_of_slot=None, period_of_day=None, host_out=None,
            defer_sync=False, state_in=None, state_out=None, forcing_error=None, keep_forcing_table=False,
            forcing_noise_in=None, forcing_noise_out=None):
        """Integrate every (member, reach) through all days on the device.

        forcing [n_sets,2,D] (rows P, PET; [n_sets,3,D] = Precipitation, PET, T_air with ``opts.snow``), doy [D], member_params [NP_M,E], reach_params [NP_R,S,E] may be numpy
        arrays or device tensors.  Returns (out [n_cols,D,n_out_reaches,E] device tensor,
        status [E] device tensor, stats dict).  ``member_rhs``: optional int32 device tensor [E] that
        receives the per-member count of right-hand-side evaluations.  With ``opts.out_slot_order`` the
        columns of ``out`` are lane slots; ``member_of_slot`` (int32 device tensor [E], allocated here when
        not given and returned in stats['member_of_slot']) maps them back to members.  With
        ``opts.n_periods`` > 0 and ``period_of_day`` [D] (int32), ``out`` has one row per period holding
        the sum of the daily values of that period.  ``host_out``: a C-contiguous float64 numpy array shaped like ``out``
        (page-locked: ``engine.pinned_empty``) that receives the table too, streamed time chunk by time chunk while the
        kernel runs (``simplyp_stream_out``); the call returns when its last byte has arrived
        (stats: ``streamed_chunks``, ``d2h_tail_ms``, ``wall_ms``).  ``defer_sync=True`` (needs a non-default torch stream
        to be current): the call returns as soon as the launches are enqueued (``simplyp_run_async``); work the caller then
        enqueues on that stream runs after the kernel but BESIDE the tail of the streamed copies; the returned dict holds only
        ``member_of_slot`` and ``finish`` -- call ``stats.update(stats.pop('finish')())`` to wait (``simplyp_sync``) and get the
        statistics.  ``state_in`` / ``state_out`` (``simplyp_set_state``): the model state ``[S, abi.N_STATE, E]`` (rows
        ``abi.STATE_ROWS``, member order) the run starts from instead of the cold initial conditions (numpy or device
        tensor), and a float64 device tensor of that shape that receives the state after the last day (``True`` allocates
        one; the same tensor may serve as both).  The end state comes back as ``stats['state']``; with ``defer_sync`` it is
        valid after ``finish``.  ``forcing_error``: forcing uncertainty -- the resolved dict of ``simplyp_amd.forcing.resolve``
        (sigma [3], groups, shift, seed, member0): every member's own forcing set is drawn on the device from ``forcing`` /
        ``forcing_of_member`` before the run's launches (``simplyp_opts.forcing_*``) into a table [E, rows, D] allocated here,
        which ``keep_forcing_table=True`` returns as ``stats['forcing_table']`` (``ValueError`` naming its size when it does not
        fit the device's free memory); ``opts`` itself is left as it is.  ``forcing_noise_in`` / ``forcing_noise_out`` (need a
        ``forcing_error`` with some ``rho > 0``): the noise state ``[6, E]`` (``abi.FORCING_NOISE_ROWS``, member order) the
        autocorrelated rows continue instead of a stationary start (numpy or device tensor), and a float64 device tensor of that
        shape that receives the state after the last day (``True`` allocates one; the same tensor may serve as both).  It comes
        back as ``stats['forcing_noise']``; with ``defer_sync`` it is valid after ``finish``.
        """
        torch = self.torch
        L = lib()
        f = self.to_device(forcing, torch.float64)
        dy = self.to_device(doy, torch.int32)
        mp = self.to_device(member_params, torch.float64)
        rp = self.to_device(reach_params, torch.float64)
        fom = None if forcing_of_member is None else self.to_device(forcing_of_member, torch.int32)
        pod = None if period_of_day is None else self.to_device(period_of_day, torch.int32)
        n_sets, two, D = f.shape
        npm, E = mp.shape
        npr, S, E2 = rp.shape
        from . import marshal
        if two != (3 if opts.snow else 2) or npm != marshal.NP_M or npr != marshal.NP_R or E2 != E or dy.shape[0] != D:
            raise ValueError("inconsistent array shapes: forcing %s doy %s member_params %s reach_params %s"
                             % (tuple(f.shape), tuple(dy.shape), tuple(mp.shape), tuple(rp.shape)))
        up_ptr = _i32(up_ptr)
        up_idx = _i32(up_idx)
        if up_ptr.shape[0] != S + 1:
            raise ValueError("up_ptr must have S+1 entries")
        oreach = _i32(out_reaches)
        n_or = S if oreach is None else len(oreach)
        ncols = bin(opts.out_mask).count('1')
        dims = abi.Dims(E, S, D, n_sets)
        rows = opts.n_periods if opts.n_periods > 0 else D
        if opts.n_periods > 0 and (pod is None or pod.shape[0] != D):
            raise ValueError("opts.n_periods > 0 needs period_of_day with one entry per day")
        if out is None:
            out = torch.empty((ncols, rows, n_or, E), dtype=torch.float64, device=self.tdev)
        elif tuple(out.shape) != (ncols, rows, n_or, E) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 device tensor of shape %s" % ((ncols, rows, n_or, E),))
        assert out.numel() * 8 == L.simplyp_out_bytes(C.byref(dims), C.byref(opts), n_or)
        if host_out is not None:
            if (not isinstance(host_out, np.ndarray) or host_out.dtype != np.float64 or not host_out.flags['C_CONTIGUOUS']
                    or host_out.shape != (ncols, rows, n_or, E)):
                raise ValueError("host_out must be a C-contiguous float64 numpy array of shape %s" % ((ncols, rows, n_or, E),))
        st_in = None
        if state_in is not None:
            st_in = state_in if (torch.is_tensor(state_in) and state_in.device == self.tdev and state_in.dtype == torch.float64
                                 and state_in.is_contiguous()) else self.to_device(state_in, torch.float64)
            if tuple(st_in.shape) != (S, abi.N_STATE, E):
                raise ValueError("state_in must have shape %s, got %s" % ((S, abi.N_STATE, E), tuple(st_in.shape)))
        if state_out is True:
            state_out = torch.empty((S, abi.N_STATE, E), dtype=torch.float64, device=self.tdev)
        elif state_out is False:
            state_out = None
        if state_out is not None and (not torch.is_tensor(state_out) or tuple(state_out.shape) != (S, abi.N_STATE, E)
                                      or state_out.dtype != torch.float64 or not state_out.is_contiguous()
                                      or state_out.device != self.tdev):
            raise ValueError("state_out must be True or a contiguous float64 tensor of shape %s on %s"
                             % ((S, abi.N_STATE, E), self.tdev))
        if state_out is not None:
            assert state_out.numel() * 8 == L.simplyp_state_bytes(C.byref(dims))
        fe_keep = None
        if forcing_noise_out is False:
            forcing_noise_out = None
        if forcing_error is not None:
            opts, fe_keep = self._forcing_opts(opts, forcing_error, E, D, two, forcing_noise_in, forcing_noise_out)
            forcing_noise_out = fe_keep[4]
        elif forcing_noise_in is not None or forcing_noise_out is not None:
            raise ValueError("forcing_noise_in / forcing_noise_out need forcing_error with some rho > 0")
        status = torch.empty((E,), dtype=torch.int32, device=self.tdev)
        if opts.out_slot_order and member_of_slot is None:
            member_of_slot = torch.empty((E,), dtype=torch.int32, device=self.tdev)
        stats = abi.Stats()
        with torch.cuda.device(self.tdev):
            self._bind_stream()
            ip = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(C.POINTER(C.c_int32))
            # the arm is one-shot and consumed by the next run whatever its outcome; disarming explicitly when no host table is
            # wanted keeps this context safe even against an arm left by another user of the same handle
            if host_out is not None:
                self._check(L.simplyp_stream_out(self._h, C.c_void_p(host_out.ctypes.data), C.c_int64(host_out.nbytes)),
                            'simplyp_stream_out')
            else:
                self._check(L.simplyp_stream_out(self._h, None, C.c_int64(0)), 'simplyp_stream_out')
            # one-shot like the stream arm; (None, None) disarms
            self._check(L.simplyp_set_state(self._h, None if st_in is None else C.c_void_p(st_in.data_ptr()),
                                            None if state_out is None else C.c_void_p(state_out.data_ptr())),
                        'simplyp_set_state')
            args = (self._h, C.byref(dims), C.byref(opts), f.data_ptr(), dy.data_ptr(),
                    None if pod is None else pod.data_ptr(),
                    None if fom is None else fom.data_ptr(), mp.data_ptr(), rp.data_ptr(),
                    ip(up_ptr), ip(up_idx), ip(oreach), n_or, out.data_ptr(), status.data_ptr(),
                    None if member_of_slot is None else member_of_slot.data_ptr(),
                    None if member_rhs is None else member_rhs.data_ptr())
            if defer_sync:
                if not torch.cuda.current_stream(self.tdev).cuda_stream:
                    raise EngineError("defer_sync needs a non-default torch stream to be current (torch.cuda.stream(...))")
                rc = L.simplyp_run_async(*args)
            else:
                rc = L.simplyp_run(*(args + (C.byref(stats),)))
        self._check(rc, 'simplyp_run')
        if defer_sync:
            keep = [f, dy, pod, fom, mp, rp, host_out, st_in, fe_keep, opts]          # inputs stay alive until the run is over

            def finish():
                with torch.cuda.device(self.tdev):
                    self._check(L.simplyp_sync(self._h, C.byref(stats)), 'simplyp_sync')
                keep.clear()
                return stats.as_dict()
            sd = {'finish': finish}
        else:
            sd = stats.as_dict()
        if member_of_slot is not None:
            sd['member_of_slot'] = member_of_slot
        if state_out is not None:
            sd['state'] = state_out
        if keep_forcing_table and fe_keep is not None:
            sd['forcing_table'] = fe_keep[0]
        if forcing_noise_out is not None:
            sd['forcing_noise'] = forcing_noise_out
        return out, status, sd

    def _forcing_opts(self, opts, fe, E, D, rows, noise_in=None, noise_out=None):
        """(a copy of ``opts`` with the forcing_* fields filled from the resolved ``fe`` and the noise state, [table, the device
        arrays they point at: groups, shift, noise in, noise out, shift groups]); the table is a view of a workspace that
        also holds the plan of a PET model behind it."""
        from . import forcing as forcing_rules
        torch = self.torch
        forcing_rules.check_resolved(fe, E, D, rows)
        n_noise = len(abi.FORCING_NOISE_ROWS)
        if (noise_in is not None or noise_out is not None) and not forcing_rules.any_rho(fe):
            raise ValueError("forcing_noise_in / forcing_noise_out need forcing_error with some rho > 0")
        if noise_in is not None:
            if not (torch.is_tensor(noise_in) and noise_in.device == self.tdev and noise_in.dtype == torch.float64 and noise_in.is_contiguous()):
                noise_in = self.to_device(noise_in, torch.float64)
            if tuple(noise_in.shape) != (n_noise, E):
                raise ValueError("forcing_noise_in must have shape %s, got %s" % ((n_noise, E), tuple(noise_in.shape)))
        if noise_out is not None and noise_out is not True and (
                not torch.is_tensor(noise_out) or tuple(noise_out.shape) != (n_noise, E) or noise_out.dtype != torch.float64
                or not noise_out.is_contiguous() or noise_out.device != self.tdev):
            raise ValueError("forcing_noise_out must be True or a contiguous float64 tensor of shape %s on %s" % ((n_noise, E), self.tdev))
        nbytes = E * rows * D * 8
        pet = fe.get('pet')
        plan_bytes = 0 if pet is None else abi.forcing_pet_plan_bytes(D)      # the plan of a PET model stands behind the table
        with torch.cuda.device(self.tdev):
            free = torch.cuda.mem_get_info(self.tdev)[0] + torch.cuda.memory_reserved(self.tdev) - torch.cuda.memory_allocated(self.tdev)
        if nbytes + plan_bytes > free:
            raise ValueError("forcing_error: the members' forcing table [E = %d, %d, D = %d] takes %d bytes (%.2f GB), the device has "
                             "%.2f GB free next to the output table -- run fewer members per call, or windows of fewer days"
                             % (E, rows, D, nbytes, nbytes / 1e9, free / 1e9))
        work = torch.empty((E * rows * D + (plan_bytes + 7) // 8,), dtype=torch.float64, device=self.tdev)
        table = work[:E * rows * D].view(E, rows, D)
        if noise_out is True:
            noise_out = torch.empty((n_noise, E), dtype=torch.float64, device=self.tdev)
        groups = [None if g is None else self.to_device(g, torch.int32) for g in fe['groups']]
        shift = None if fe.get('shift') is None else self.to_device(fe['shift'], torch.float64)
        sgroups = None if fe.get('shift_groups') is None else self.to_device(fe['shift_groups'], torch.int32)
        o = opts.copy()
        o.forcing_error = 1
        o.forcing_member0 = int(fe.get('member0', 0))
        o.forcing_seed = int(fe.get('seed', 0))
        for r in range(3):
            o.forcing_sigma[r] = float(fe['sigma'][r])
            o.forcing_group_of_day[r] = None if groups[r] is None else groups[r].data_ptr()
        o.forcing_shift = None if shift is None else shift.data_ptr()
        o.forcing_shift_rows = 0 if shift is None else int(shift.shape[0])
        o.forcing_table = table.data_ptr()
        for r in range(3):
            o.forcing_rho[r] = 0.0 if fe.get('rho') is None else float(fe['rho'][r])
        o.forcing_noise_in = None if noise_in is None else noise_in.data_ptr()
        o.forcing_noise_out = None if noise_out is None else noise_out.data_ptr()
        o.forcing_shift_group_of_day = None if sgroups is None else sgroups.data_ptr()
        o.forcing_shift_groups = 0 if sgroups is None else int(shift.shape[1])
        if pet is not None:                                      # daylight [M], month [2, M], day [3, D]: include/simplyp.h
            M = int(pet['months'])
            assert M == 12 * (D // 365) and len(pet['node']) == D
            tail = work[E * rows * D:]
            tail[:M] = self.to_device(pet['daylight'], torch.float64)
            ints = tail[M:].view(torch.int32)
            ints[:2 * M] = self.to_device(np.concatenate([pet['first'], pet['days']]), torch.int32)
            ints[2 * M:2 * M + 3 * D] = self.to_device(np.concatenate([pet['node'], pet['k'], pet['n']]), torch.int32)
            o.forcing_pet_model = int(pet['model'])
        return o, [table, groups, shift, noise_in, noise_out, sgroups]


    def eval_units(self, which, rows):
        """The path's scalar device functions on given arguments (``simplyp_eval_units``): ``which`` = 'f_x' (rows [n, 2] =
        x, threshold -> [n, 2]: the gate as the end-of-day flows and as the right-hand side evaluate it) or 'soilp' (rows
        [n, 10] = the arguments of the reference's discretized_soilP -> [n, 3] = TDPs, Plab, conc_TDPs); and the fp64
        elementary functions every kernel calls: 'exp' (rows [n, 1] = x -> [n, 4]: exp(x) evaluated alone, in slot 1 of a group
        of two, in slots 0 and 6 of a group of seven), 'log' (rows [n, 1] -> [n, 1]), 'rcp' (rows [n, 1] -> [n, 3]: the raw
        hardware reciprocal, one Newton step, two Newton steps) and 'pow' (rows [n, 2] = q, b -> [n, 1] = exp(b log(q))); and
        'rhs' (rows [n, 51] = the 8 carried states and the 43 parameters of ode_f -> [n, 77]: the literal, the augmented, the
        four-lane and the fp32 statement of the right-hand side) and 'step' (rows [n, 19] = the arguments of the five pieces of
        the step rule -> [n, 11]); the columns are listed at ``simplyp_eval_units`` in include/simplyp.h."""
        torch = self.torch
        w, k_in, k_out = {'f_x': (0, 2, 2), 'soilp': (1, 10, 3), 'exp': (2, 1, 4), 'log': (3, 1, 1), 'rcp': (4, 1, 3),
                           'pow': (5, 2, 1), 'rhs': (6, 51, 77), 'step': (7, 19, 11)}[which]
        a = self.to_device(np.ascontiguousarray(rows, dtype=np.float64), torch.float64)
        if a.dim() != 2 or a.shape[1] != k_in:
            raise ValueError("%s takes rows of %d values" % (which, k_in))
        out = torch.empty((a.shape[0], k_out), dtype=torch.float64, device=self.tdev)
        self._info_call(None, 'simplyp_eval_units', self._h, w, a.shape[0], a.data_ptr(), out.data_ptr())
        return out.cpu().numpy()

    def order_members(self, cost, where='device', diag=False, keys=False):
        """The members' lane-slot order of a balanced run from a given cost table (``simplyp_order_members``): ``cost`` [8, E]
        (anything numpy turns into uint32, or an int32 device tensor holding the same bits), ``where`` = 'device' (the kernels a
        balanced run launches) or 'host' (the host rule on a copy).  Returns the permutation [E] as a numpy int32 array, or a
        tuple that starts with it when more is asked for: ``diag=True`` adds the [68] doubles mean[8], 1 / deviation[8], the 36
        covariances (i <= j, row by row), v2[8], v3[8]; ``keys=True`` ('device' only) the [E] sorted total-cost keys as
        uint64."""
        torch = self.torch
        w = {'device': 0, 'host': 1}[where]
        if torch.is_tensor(cost):
            c = cost
            if c.dtype != torch.int32 or c.device != self.tdev or not c.is_contiguous():
                raise ValueError("a cost tensor must be a contiguous int32 tensor on %s" % self.tdev)
        else:
            c = self.to_device(np.ascontiguousarray(cost, dtype=np.uint32).view(np.int32))
        if c.dim() != 2 or c.shape[0] != 8:
            raise ValueError("cost must have shape [8, E], got %s" % (tuple(c.shape),))
        E = int(c.shape[1])
        perm = torch.empty((max(E, 1),), dtype=torch.int32, device=self.tdev)
        d = torch.empty((68,), dtype=torch.float64, device=self.tdev) if diag else None
        k = torch.empty((max(E, 1),), dtype=torch.int64, device=self.tdev) if keys else None
        self._info_call(None, 'simplyp_order_members', self._h, E, c.data_ptr(), w, perm.data_ptr(), self._ptr(d), self._ptr(k))
        got = [perm.cpu().numpy()]
        if diag:
            got.append(d.cpu().numpy())
        if keys:
            got.append(k.cpu().numpy().view(np.uint64))
        return got[0] if len(got) == 1 else tuple(got)

    # ---- what the analysis methods do alike ----
    def _info_call(self, info_class, name, *args, bind=True):
        """The library entry ``name`` with a fresh ``info_class`` as its last argument (None: the entry takes none), on this
        engine's device and ordered after torch's current stream (``bind=False``: a second entry of one public method, which the
        first has bound already -- ``_bind_stream`` may synchronise).  Raises EngineError unless the entry returns 0; returns the
        info as a dict."""
        info = None if info_class is None else info_class()
        with self.torch.cuda.device(self.tdev):
            if bind:
                self._bind_stream()
            rc = getattr(lib(), name)(*(args if info is None else args + (C.byref(info),)))
        self._check(rc, name)
        return None if info is None else info.as_dict()

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def _member_table(self, table):
        """(E, lead, n_rows) of a table whose LAST axis is the member axis: its members, the shape of its rows, their number."""
        torch = self.torch
        if not torch.is_tensor(table) or table.dtype != torch.float64 or not table.is_contiguous() or table.dim() < 1 \
                or table.device != self.tdev:
            raise ValueError("table must be a contiguous float64 tensor on %s whose last axis is the member axis" % (self.tdev,))
        lead = tuple(int(x) for x in table.shape[:-1])
        return int(table.shape[-1]), lead, (int(np.prod(lead, dtype=np.int64)) if lead else 1)

    def _f_tdp(self, f_tdp, E):
        torch = self.torch
        ft = self.to_device(np.ascontiguousarray(np.broadcast_to(np.asarray(f_tdp, dtype=np.float64), (E,)))
                            if not torch.is_tensor(f_tdp) else f_tdp, torch.float64)
        if tuple(ft.shape) != (E,):
            raise ValueError("f_tdp must be a scalar or have one entry per member")
        return ft

    @staticmethod
    def _q_array(q):
        qa = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=np.float64)))
        if qa.ndim != 1:
            raise ValueError("q must be a list of probabilities")
        return qa

    def _include_mask(self, include, E):
        torch = self.torch
        if include is None:
            return None
        inc = include if torch.is_tensor(include) else torch.from_numpy(np.ascontiguousarray(np.asarray(include) != 0))
        inc = (inc != 0).to(torch.uint8).to(self.tdev).contiguous()
        if tuple(inc.shape) != (E,):
            raise ValueError("include must have one entry per member")
        return inc

    def _check_member_of_slot(self, member_of_slot, E):
        if member_of_slot is not None and (member_of_slot.dtype != self.torch.int32 or tuple(member_of_slot.shape) != (E,)):
            raise ValueError("member_of_slot must be an int32 device tensor with one entry per member")

    def _daily_table(self, out, out_mask, reach_params, out_reaches, member_of_slot, need_reach_params=False):
        """The daily table ``out`` [n_cols, D, n_reaches, E] of a previous ``run`` and what comes with it, checked against each
        other: ``out_mask``, ``out_reaches``, ``reach_params`` (to the device; may be None unless ``need_reach_params``) and
        ``member_of_slot``.  Returns (head, rp, (D, n_reaches, E), keep): the arguments every table entry of the library starts
        with, the device copy of ``reach_params``, the sizes, and what must stay alive until the call is over."""
        torch = self.torch
        if not torch.is_tensor(out) or out.dim() != 4 or out.dtype != torch.float64 or not out.is_contiguous() \
                or out.device != self.tdev:
            raise ValueError("out must be a contiguous float64 tensor [n_cols, D, n_reaches, E] on %s" % (self.tdev,))
        ncols, D, n_or, E = (int(x) for x in out.shape)
        oreach = _i32(out_reaches)
        if need_reach_params and reach_params is None:
            raise ValueError("reach_params [NP_R, S, E] is needed")
        rp = None if reach_params is None else self.to_device(reach_params, torch.float64)
        S = int(rp.shape[1]) if rp is not None else (n_or if oreach is None else max(n_or, int(oreach.max()) + 1))
        if ncols != bin(out_mask).count('1') or n_or != (S if oreach is None else len(oreach)) \
                or (rp is not None and int(rp.shape[2]) != E):
            raise ValueError("out %s does not match out_mask / out_reaches / reach_params %s"
                             % (tuple(out.shape), None if rp is None else tuple(rp.shape)))
        self._check_member_of_slot(member_of_slot, E)
        dims = abi.Dims(E, S, D, 1)
        head = (self._h, C.byref(dims), int(out_mask), None if oreach is None else oreach.ctypes.data_as(C.POINTER(C.c_int32)), n_or,
                out.data_ptr(), self._ptr(member_of_slot))
        return head, rp, (D, n_or, E), [dims, oreach, rp]

    def gof(self, out, out_mask, obs, f_tdp, reach_params, out_reaches=None, member_of_slot=None, spearman=False, gof=None):
        """Per-member goodness-of-fit statistics (the reference's ``goodness_of_fit_stats``,
        visualise_results.py:387-474, without Spearman's r) of the daily table ``out`` of a previous ``run``.

        out [n_cols,D,n_out_reaches,E] device tensor written with ``out_mask`` (must contain Qr and the three daily
        fluxes); obs [n_out_reaches,6,D] host array, NaN = no observation (``visualise_results.observation_array``);
        f_tdp [E] or scalar; reach_params [NP_R,S,E].  Returns (gof [n_stats,6,n_out_reaches,E] device tensor in member
        order -- rows ``abi.GOF_STATS``, variables ``abi.GOF_VARS`` -- and an info dict).  ``spearman=True`` adds the rank
        correlation (``simplyp_gof_spearman``, the remaining column of the reference's table) as
        ``info['spearman']`` [6, n_out_reaches, E] device tensor and its cost as ``info['spearman_ms']``.  ``gof``: a
        float64 device tensor of the result's shape to write into instead of a new one (a loop that reduces run after run)."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot, True)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.shape != (n_or, len(abi.GOF_VARS), D):
            raise ValueError("obs must have shape %s, got %s" % ((n_or, len(abi.GOF_VARS), D), obs.shape))
        ft = self._f_tdp(f_tdp, E)
        shape = (len(abi.GOF_STATS), len(abi.GOF_VARS), n_or, E)
        if gof is None:
            gof = torch.empty(shape, dtype=torch.float64, device=self.tdev)
        elif tuple(gof.shape) != shape or gof.dtype != torch.float64 or not gof.is_contiguous() or gof.device != self.tdev:
            raise ValueError("gof must be a contiguous float64 tensor of shape %s on %s" % (shape, self.tdev))
        tail = (ft.data_ptr(), rp.data_ptr(), obs.ctypes.data_as(C.POINTER(C.c_double)))
        d = self._info_call(abi.GofInfo, 'simplyp_gof', *(head + tail + (gof.data_ptr(),)))
        if spearman:
            rho = torch.empty((len(abi.GOF_VARS), n_or, E), dtype=torch.float64, device=self.tdev)
            sinfo = self._info_call(abi.GofInfo, 'simplyp_gof_spearman', *(head + tail + (rho.data_ptr(),)), bind=False)
            d['spearman'] = rho
            d['spearman_ms'] = sinfo['kernel_ms']
        del keep
        return gof, d

    def gof_lag(self, out, out_mask, obs, f_tdp, reach_params, out_reaches=None, member_of_slot=None, lag=None):
        """Per-member lag-one sums of the relative residuals ``obs / sim - 1`` (``simplyp_gof_lag``; ``simplyp_amd.residuals``
        states them) of the daily table ``out`` of a previous ``run``.  Arguments as for ``gof``.  Returns (lag
        [4, 6, n_out_reaches, E] device tensor in member order -- rows ``abi.LAG_STATS``, variables ``abi.GOF_VARS``, NaN rows for
        variables with 10 or fewer observations -- and an info dict).  ``lag``: a tensor of that shape to write into."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot, True)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.shape != (n_or, len(abi.GOF_VARS), D):
            raise ValueError("obs must have shape %s, got %s" % ((n_or, len(abi.GOF_VARS), D), obs.shape))
        ft = self._f_tdp(f_tdp, E)
        shape = (len(abi.LAG_STATS), len(abi.GOF_VARS), n_or, E)
        if lag is None:
            lag = torch.empty(shape, dtype=torch.float64, device=self.tdev)
        elif tuple(lag.shape) != shape or lag.dtype != torch.float64 or not lag.is_contiguous() or lag.device != self.tdev:
            raise ValueError("lag must be a contiguous float64 tensor of shape %s on %s" % (shape, self.tdev))
        d = self._info_call(abi.GofInfo, 'simplyp_gof_lag', *(head + (ft.data_ptr(), rp.data_ptr(),
                                                                      obs.ctypes.data_as(C.POINTER(C.c_double)), lag.data_ptr())))
        del keep
        return lag, d

    def waterbody(self, out, out_mask, sum_reaches, f_tdp, reach_params, out_reaches=None, member_of_slot=None,
                  columns=None):
        """The reference's ``sum_to_waterbody`` (model.py:851-900) for every member, on the device, from the daily table
        ``out`` of a previous ``run`` (written with ``out_mask``: must contain Qr and the three daily fluxes).

        sum_reaches: zero-based ids of the reaches flagged 'In_final_flux?' (ascending; each must be an output reach of
        the table); f_tdp scalar or [E]; reach_params [NP_R,S,E]; columns: names from ``abi.WB_COLUMNS`` (default all 11).
        Returns (wb [n_columns, D, E] device tensor, member axis ordered like ``out``'s, and an info dict)."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot, True)
        cols = list(abi.WB_COLUMNS) if columns is None else list(columns)
        wb_mask = sum(1 << abi.WB_COLUMNS.index(c) for c in cols)
        cols = [c for c in abi.WB_COLUMNS if c in cols]
        sr = _i32(sum_reaches)
        ft = self._f_tdp(f_tdp, E)
        wb = torch.empty((len(cols), D, E), dtype=torch.float64, device=self.tdev)
        d = self._info_call(abi.WbInfo, 'simplyp_waterbody',
                            *(head + (ft.data_ptr(), rp.data_ptr(), sr.ctypes.data_as(C.POINTER(C.c_int32)), len(sr), wb_mask,
                                      wb.data_ptr())))
        del keep
        d['columns'] = cols
        return wb, d

    def gof_waterbody(self, wb, columns, obs, f_tdp, member_of_slot=None):
        """``gof`` for the summed series: wb [n_columns, D, E] from ``waterbody`` (``columns`` as returned there, must hold
        Q_cumecs and the three summed fluxes); obs [6, D] host array.  Returns (gof [n_stats, 6, 1, E], info)."""
        torch = self.torch
        ncols, D, E = wb.shape
        wb_mask = sum(1 << abi.WB_COLUMNS.index(c) for c in columns)
        if ncols != len(columns) or wb.dtype != torch.float64 or not wb.is_contiguous():
            raise ValueError("wb %s does not match columns %s" % (tuple(wb.shape), columns))
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.shape != (len(abi.GOF_VARS), D):
            raise ValueError("obs must have shape %s, got %s" % ((len(abi.GOF_VARS), D), obs.shape))
        ft = self._f_tdp(f_tdp, E)
        gof = torch.empty((len(abi.GOF_STATS), len(abi.GOF_VARS), 1, E), dtype=torch.float64, device=self.tdev)
        dims = abi.Dims(E, 1, D, 1)
        info = self._info_call(abi.GofInfo, 'simplyp_gof_waterbody', self._h, C.byref(dims), wb_mask, wb.data_ptr(),
                               self._ptr(member_of_slot), ft.data_ptr(), obs.ctypes.data_as(C.POINTER(C.c_double)), gof.data_ptr())
        return gof, info

    def quantiles(self, table, q, include=None, member_of_slot=None):
        """Exact order statistics across the member axis (``simplyp_quantiles``): the two values that bracket numpy's
        ``method='linear'`` quantile of every row, selected on the device; the table is only read.

        table: contiguous float64 device tensor whose LAST axis is the member axis (a run's ``out``, daily or reduced, a
        waterbody table, a goodness-of-fit table); q: probabilities in [0, 1], at most 16; include: optional [E] mask in
        member order (bool / uint8, numpy or device tensor) -- members with 0 take part in no row; member_of_slot: the int32
        device tensor of a run that wrote slot order (``include`` is looked up through it).
        Returns (lower, upper, info): device tensors of shape ``(K,) + table.shape[:-1]`` holding x_(floor(h)) and
        x_(min(floor(h) + 1, n - 1)), h = q (n - 1), n = ``info['n_used']``; ``interpolate_quantiles`` turns them into
        numpy's values.  All NaN when no member is included."""
        torch = self.torch
        E, lead, n_rows = self._member_table(table)
        qa = self._q_array(q)
        K = len(qa)
        inc = self._include_mask(include, E)
        self._check_member_of_slot(member_of_slot, E)
        stats = torch.empty((2, max(K, 1)) + lead, dtype=torch.float64, device=self.tdev)
        info = self._info_call(abi.QuantileInfo, 'simplyp_quantiles', self._h, E, n_rows, table.data_ptr(), self._ptr(member_of_slot),
                               self._ptr(inc), qa.ctypes.data_as(C.POINTER(C.c_double)), K, stats.data_ptr())
        return stats[0], stats[1], info

    def _weight_vector(self, weights, E):
        """Integer weights [E] in member order (numpy integers or an int64 device tensor, e.g. ``pf_weights``' q) as a contiguous
        int64 device tensor: the library reads them as uint64 and checks their values."""
        torch = self.torch
        if torch.is_tensor(weights):
            if weights.dtype != torch.int64:
                raise ValueError("weights must be an int64 tensor (pf_weights' q) or an integer array")
            wt = weights.to(self.tdev).contiguous()
        else:
            wa = np.asarray(weights)
            if wa.dtype.kind not in 'iu':
                raise ValueError("weights must be integers (weighted.linear_weights, particle.weights(...)['q'])")
            if wa.size and (int(wa.min()) < 0 or int(wa.max()) >= 1 << 63):
                raise ValueError("weights must lie in [0, 2^40]")
            wt = torch.from_numpy(np.ascontiguousarray(wa.astype(np.int64))).to(self.tdev)
        if tuple(wt.shape) != (E,):
            raise ValueError("weights must have one entry per member")
        return wt

    def weighted_quantiles(self, table, q, weights, include=None, member_of_slot=None):
        """Exact quantiles across the member axis under integer weights (``simplyp_weighted_quantiles``; ``simplyp_amd.weighted``
        states the rule): for every row and probability the value of the first member, in ``quantiles``' order, whose running
        weight reaches ``max(1, ceil(p T))`` -- numpy's ``method='inverted_cdf'`` with ``weights=``, one value per probability.

        table, q, include, member_of_slot as for ``quantiles``; weights: [E] integers in MEMBER order, each in [0, 2^40] (numpy,
        or the int64 device tensor ``pf_weights`` returns); a member with weight 0 takes no part.
        Returns (values, info): a device tensor of shape ``(K,) + table.shape[:-1]`` and a dict with ``T`` (the participating
        weights' sum), ``n_used`` and ``n_passes``.  All NaN when ``T`` is 0."""
        torch = self.torch
        E, lead, n_rows = self._member_table(table)
        qa = self._q_array(q)
        K = len(qa)
        inc = self._include_mask(include, E)
        self._check_member_of_slot(member_of_slot, E)
        wt = self._weight_vector(weights, E)
        values = torch.empty((max(K, 1),) + lead, dtype=torch.float64, device=self.tdev)
        info = self._info_call(abi.WqInfo, 'simplyp_weighted_quantiles', self._h, E, n_rows, table.data_ptr(), self._ptr(member_of_slot),
                               self._ptr(inc), wt.data_ptr(), qa.ctypes.data_as(C.POINTER(C.c_double)), K, values.data_ptr())
        return values, info

    def time_quantiles(self, out, out_mask, q, series=None, period_of_day=None, f_tdp=None, reach_params=None,
                       out_reaches=None, member_of_slot=None, n_periods=None):
        """Exact order statistics per member along the DAY axis (``simplyp_time_quantiles``) of the daily table ``out``
        [n_cols, D, n_reaches, E] of a previous ``run`` (written with ``out_mask``): the two values that bracket numpy's
        ``method='linear'`` quantile of every member's series over each period, selected on the device; the table is only read.

        q: probabilities in [0, 1], at most 16.  series: ids -- ``SIMPLYP_OUT_*`` column numbers (in ``out_mask``) or
        ``abi.TQ_DERIVED + abi.GOF_VARS.index(v)`` for the df_R series Q_cumecs, SS_mgl, TDP_mgl, PP_mgl, TP_mgl, SRP_mgl,
        which need ``f_tdp`` (scalar or [E]) and ``reach_params`` [NP_R, S, E]; default: every column of the mask.
        period_of_day: int array [D] in [-1, n_periods), -1 = the day takes part in no period, the others non-decreasing;
        None = one period holding every day; n_periods: their number when periods past the last named one exist (default:
        the largest entry + 1).  Without ``reach_params`` the table's reaches are all S reaches or the
        ``out_reaches`` given.
        Returns (lower, upper, info): device tensors [K, n_series, P, n_reaches, E], member axis ordered like ``out``'s, holding
        x_(floor(h)) and x_(min(floor(h) + 1, n - 1)), h = q (n - 1), n = ``info['n_days'][p]`` (NaN where n = 0);
        ``interpolate_time_quantiles`` turns them into numpy's values."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot)
        qa = self._q_array(q)
        K = len(qa)
        sa = np.ascontiguousarray([c for c in range(32) if (out_mask >> c) & 1] if series is None else series, dtype=np.int32)
        if sa.ndim != 1:
            raise ValueError("series must be a list of series ids")
        pod, P = None, 0
        if period_of_day is not None:
            pod = np.ascontiguousarray(period_of_day, dtype=np.int32)
            if pod.shape != (D,):
                raise ValueError("period_of_day needs one entry per day")
            P = max(int(pod.max()) + 1, 1) if D > 0 else 1
            P = P if n_periods is None else int(n_periods)
        ft = None if f_tdp is None else self._f_tdp(f_tdp, E)
        stats = torch.empty((2, max(K, 1), max(len(sa), 1), max(P, 1), n_or, E), dtype=torch.float64, device=self.tdev)
        n_days = np.zeros(max(P, 1), dtype=np.int32)
        i32 = C.POINTER(C.c_int32)
        d = self._info_call(abi.TqInfo, 'simplyp_time_quantiles',
                            *(head + (self._ptr(ft), self._ptr(rp), sa.ctypes.data_as(i32), len(sa),
                                      None if pod is None else pod.ctypes.data_as(i32), P, qa.ctypes.data_as(C.POINTER(C.c_double)), K,
                                      stats.data_ptr(), n_days.ctypes.data_as(i32))))
        del keep
        d['n_days'] = n_days
        return stats[0], stats[1], d

    def _predictive_args(self, out, out_mask, series, err_m, f_tdp, reach_params, out_reaches, member_of_slot):
        """The arguments ``predictive_series`` and ``predictive_bands`` share, checked and on the device."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot)
        sa = np.ascontiguousarray(series, dtype=np.int32)
        if sa.ndim != 1:
            raise ValueError("series must be a list of series ids")
        em = None
        if err_m is not None:
            if not torch.is_tensor(err_m):
                err_m = np.ascontiguousarray(np.broadcast_to(np.asarray(err_m, dtype=np.float64), (len(sa), E)))
            em = self.to_device(err_m, torch.float64)
            if tuple(em.shape) != (len(sa), E):
                raise ValueError("err_m must be a scalar or [n_series, E] (member order)")
        ft = None if f_tdp is None else self._f_tdp(f_tdp, E)
        tail = (self._ptr(ft), self._ptr(rp), sa.ctypes.data_as(C.POINTER(C.c_int32)), len(sa), self._ptr(em))
        return head, tail, (len(sa), D, n_or, E), keep + [sa, em, ft]

    def predictive_series(self, out, out_mask, series, err_m=None, seed=0, day0=0, normals=False, f_tdp=None,
                          reach_params=None, out_reaches=None, member_of_slot=None):
        """The series a predictive band is taken over, materialised (``simplyp_predictive_series``): from the daily table
        ``out`` [n_cols, D, n_reaches, E] of a previous ``run`` the named ``series`` (ids as for ``time_quantiles``), with the
        reference's error model ``v + norm(0, m v)`` drawn on the device when ``err_m`` (a scalar or [n_series, E] in member
        order) is given -- individual noisy realisations of every member.  The draw is a pure function of (``seed``, member,
        ``day0`` + d, model reach, series id): ``simplyp_amd.predictive`` restates it.  ``normals=True`` returns the standard
        normals z instead of the values.  Returns a device tensor [n_series, D, n_reaches, E], member axis ordered like ``out``'s."""
        torch = self.torch
        head, tail, shape, keep = self._predictive_args(out, out_mask, series, err_m, f_tdp, reach_params, out_reaches, member_of_slot)
        table = torch.empty(shape, dtype=torch.float64, device=self.tdev)
        self._info_call(None, 'simplyp_predictive_series',
                        *(head + tail + (C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(day0), 1 if normals else 0, table.data_ptr())))
        del keep
        return table

    def predictive_bands(self, out, out_mask, q, series, err_m=None, seed=0, day0=0, include=None, f_tdp=None,
                         reach_params=None, out_reaches=None, member_of_slot=None, weights=None):
        """Order statistics across the members of the series ``predictive_series`` would write, for every (series, day,
        reach) (``simplyp_predictive_bands``): the reference's overall predictive band with ``err_m``, the parameter-only
        band of the series without.  The series are generated and selected chunk by chunk on the device; the table is only
        read.  ``q``, ``include`` and the rank rule as for ``quantiles``.  Returns (lower, upper, info): device tensors
        [K, n_series, D, n_reaches]; ``interpolate_quantiles`` with ``info['n_used']`` turns them into numpy's values.
        ``weights`` ([E] integers in member order, as for ``weighted_quantiles``): the bands under these weights instead
        (``simplyp_predictive_bands_weighted``) -- returns (values [K, n_series, D, n_reaches], info) by ``weighted_quantiles``' rule."""
        torch = self.torch
        head, tail, shape, keep = self._predictive_args(out, out_mask, series, err_m, f_tdp, reach_params, out_reaches, member_of_slot)
        E = shape[3]
        qa = self._q_array(q)
        inc = self._include_mask(include, E)
        if weights is not None:
            wt = self._weight_vector(weights, E)
            values = torch.empty((max(len(qa), 1),) + shape[:3], dtype=torch.float64, device=self.tdev)
            winfo = self._info_call(abi.WqInfo, 'simplyp_predictive_bands_weighted',
                                    *(head + (self._ptr(inc),) + tail + (C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(day0),
                                                                          qa.ctypes.data_as(C.POINTER(C.c_double)), len(qa),
                                                                          wt.data_ptr(), values.data_ptr())))
            del keep
            return values, winfo
        stats = torch.empty((2, max(len(qa), 1)) + shape[:3], dtype=torch.float64, device=self.tdev)
        info = self._info_call(abi.PredInfo, 'simplyp_predictive_bands',
                               *(head + (self._ptr(inc),) + tail + (C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(day0),
                                                                     qa.ctypes.data_as(C.POINTER(C.c_double)), len(qa), stats.data_ptr())))
        del keep
        return stats[0], stats[1], info


    def scores(self, table, y, weights=None, include=None, member_of_slot=None):
        """CRPS terms and PIT counts of every row of ``table`` against the observations ``y`` (``simplyp_scores``;
        ``simplyp_amd.score`` states the rule).  table, include, member_of_slot as for ``quantiles``; weights as for
        ``weighted_quantiles`` or None (every included member weighs 1); y: host array of shape ``table.shape[:-1]``, NaN = the
        row is not scored, +-inf is refused.
        Returns (sums, counts, info): device tensors of shape ``(2,) + table.shape[:-1]`` -- float64 ``abs_err`` and ``spread``
        (CRPS = sums[0] - sums[1]), int64 ``below`` and ``at_or_below`` -- and a dict with ``T``, ``n_used``, ``n_rows_scored``,
        ``n_chunks``, ``kernel_ms``, ``sort_ms``.  Rows without an observation and every row when ``T`` is 0: NaN and 0."""
        torch = self.torch
        E, lead, n_rows = self._member_table(table)
        ya = np.asarray(y, dtype=np.float64)
        if ya.shape != lead:
            raise ValueError("y must have one observation per row of the table: shape %s" % (lead,))
        ya = np.ascontiguousarray(ya).reshape(-1)                    # (a 0-d array too)
        inc = self._include_mask(include, E)
        self._check_member_of_slot(member_of_slot, E)
        wt = None if weights is None else self._weight_vector(weights, E)
        sums = torch.empty((2,) + lead, dtype=torch.float64, device=self.tdev)
        counts = torch.empty((2,) + lead, dtype=torch.int64, device=self.tdev)
        info = self._info_call(abi.ScoreInfo, 'simplyp_scores', self._h, E, n_rows, table.data_ptr(), self._ptr(member_of_slot),
                               self._ptr(inc), self._ptr(wt), ya.ctypes.data_as(C.POINTER(C.c_double)), sums.data_ptr(),
                               counts.data_ptr())
        return sums, counts, info

    def predictive_scores(self, out, out_mask, series, obs, err_m=None, seed=0, day0=0, include=None, weights=None, f_tdp=None,
                          reach_params=None, out_reaches=None, member_of_slot=None):
        """The scores of the series ``predictive_series`` would write against ``obs`` [n_series, D, n_reaches] (host, NaN = no
        observation), without materialising them (``simplyp_predictive_scores``): only the observed rows are generated, chunk
        by chunk, and scored by ``scores``' kernels -- the same bits as ``scores(predictive_series(...), obs)``.  Arguments as
        for ``predictive_bands``; ``weights`` None or [E] integers in member order.
        Returns (sums, counts, info) as ``scores`` does, of shape [2, n_series, D, n_reaches]."""
        torch = self.torch
        head, tail, shape, keep = self._predictive_args(out, out_mask, series, err_m, f_tdp, reach_params, out_reaches, member_of_slot)
        E = shape[3]
        oa = np.ascontiguousarray(obs, dtype=np.float64)
        if oa.shape != tuple(shape[:3]):
            raise ValueError("obs must have shape [n_series, D, n_reaches] = %s" % (tuple(shape[:3]),))
        inc = self._include_mask(include, E)
        wt = None if weights is None else self._weight_vector(weights, E)
        sums = torch.empty((2,) + tuple(shape[:3]), dtype=torch.float64, device=self.tdev)
        counts = torch.empty((2,) + tuple(shape[:3]), dtype=torch.int64, device=self.tdev)
        info = self._info_call(abi.ScoreInfo, 'simplyp_predictive_scores',
                               *(head + (self._ptr(inc),) + tail + (C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), int(day0), self._ptr(wt),
                                                                     oa.ctypes.data_as(C.POINTER(C.c_double)), sums.data_ptr(),
                                                                     counts.data_ptr())))
        del keep
        return sums, counts, info

    def pareto(self, obj, sense, include=None, member_of_slot=None, max_fronts=0, counts=True, rank=True):
        """Pareto dominance among the members on the objectives ``obj`` (``simplyp_pareto``; ``simplyp_amd.pareto`` states the
        rule).  obj: contiguous float64 device tensor [M, E], 1 <= M <= 8, the member axis last and in the column order of the
        table it came from; sense: M values, +1 = larger is better, -1 = smaller is better; include, member_of_slot as for
        ``quantiles``; max_fronts: 0 resolves every rank, F > 0 the ranks 0 .. F-1 (deeper members get ``abi.PARETO_UNRANKED``).
        ``counts=False`` / ``rank=False`` leave those outputs out (without ``rank`` no front is peeled).
        Returns a dict: int32 device tensors [E] in member order ``dominated_by``, ``dominates`` (with ``counts``) and ``rank``
        (with ``rank``) -- ``abi.PARETO_EXCLUDED`` for a member that is masked out or has a NaN objective -- and the info fields
        ``n_used``, ``n_fronts``, ``n_front0``, ``n_unranked``, ``pair_tests``, ``kernel_ms``."""
        torch = self.torch
        if not torch.is_tensor(obj) or obj.dtype != torch.float64 or not obj.is_contiguous() or obj.dim() != 2 \
                or obj.device != self.tdev:
            raise ValueError("obj must be a contiguous float64 tensor [M, E] on %s" % (self.tdev,))
        M, E = (int(x) for x in obj.shape)
        sa = np.ascontiguousarray(np.atleast_1d(np.asarray(sense)).astype(np.int32))
        if sa.shape != (M,):
            raise ValueError("sense must have one entry per objective")
        if not counts and not rank:
            raise ValueError("counts and rank are both off: nothing to compute")
        inc = self._include_mask(include, E)
        self._check_member_of_slot(member_of_slot, E)
        new = lambda: torch.empty((E,), dtype=torch.int32, device=self.tdev)
        by, of, rk = (new() if counts else None), (new() if counts else None), (new() if rank else None)
        info = self._info_call(abi.ParetoInfo, 'simplyp_pareto', self._h, E, M, obj.data_ptr(), sa.ctypes.data_as(C.POINTER(C.c_int32)),
                               self._ptr(member_of_slot), self._ptr(inc), int(max_fronts), self._ptr(by), self._ptr(of), self._ptr(rk))
        res = dict(info)
        if counts:
            res['dominated_by'], res['dominates'] = by, of
        if rank:
            res['rank'] = rk
        return res

    # ---- the stretch move (simplyp_mcmc_*; simplyp_amd.mcmc restates it) ----
    def mcmc_propose(self, theta, half, t, lo, hi, target, prop, inside, member_params=None, f_tdp=None, a=2.0, seed=0):
        """The proposals of half ``half`` at absolute step ``t`` (``simplyp_mcmc_propose``).  theta [n_dim, W] float64 device
        tensor (read); lo / hi [n_dim] the prior box and target [n_dim] (a row of ``marshal.PM_NAMES``,
        ``abi.MCMC_TARGET_F_TDP`` or ``abi.MCMC_TARGET_NONE``) on the host; prop [n_dim, W/2] float64, inside [W/2] int32,
        member_params [NP_M, W/2] and f_tdp [W/2] device tensors that are written.  The library checks the values; the tensors'
        shapes are the caller's.  Returns the info dict."""
        n_dim, W = (int(x) for x in theta.shape)
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        tg = np.ascontiguousarray(target, dtype=np.int32)
        if lo.shape != (n_dim,) or hi.shape != (n_dim,) or tg.shape != (n_dim,):
            raise ValueError("lo, hi and target need one entry per dimension")
        dbl = C.POINTER(C.c_double)
        return self._info_call(abi.McmcInfo, 'simplyp_mcmc_propose', self._h, W, n_dim, int(half), float(a),
                               C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(t) & 0xFFFFFFFF),
                               lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), tg.ctypes.data_as(C.POINTER(C.c_int32)),
                               theta.data_ptr(), self._ptr(prop), self._ptr(inside), self._ptr(member_params), self._ptr(f_tdp))

    def mcmc_log_prob(self, gof, pairs, m_dim, m_const, prop, lp_prop, status=None, inside=None):
        """The log posterior of the run points from a goodness-of-fit table (``simplyp_mcmc_log_prob``).  gof
        [n_stats, 6, n_reaches, h] as ``Engine.gof`` returns it; pairs: list of (variable index in ``abi.GOF_VARS``, position among
        the output reaches); m_dim [6]: the row of ``prop`` holding the variable's ``m`` or -1 for ``m_const[v]``; prop
        [n_dim, h]; lp_prop [h] float64 device tensor (written); status / inside [h] int32 device tensors or None."""
        n_dim, h = (int(x) for x in prop.shape)
        pv = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        pr = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        md = np.ascontiguousarray(m_dim, dtype=np.int32)
        mc = np.ascontiguousarray(m_const, dtype=np.float64)
        if md.shape != (len(abi.GOF_VARS),) or mc.shape != (len(abi.GOF_VARS),):
            raise ValueError("m_dim and m_const need one entry per variable of abi.GOF_VARS")
        if gof.dim() != 4 or tuple(gof.shape[:2]) != (len(abi.GOF_STATS), len(abi.GOF_VARS)) or int(gof.shape[3]) != h \
                or not gof.is_contiguous():
            raise ValueError("gof %s does not match prop %s" % (tuple(gof.shape), tuple(prop.shape)))
        i32 = C.POINTER(C.c_int32)
        return self._info_call(abi.McmcInfo, 'simplyp_mcmc_log_prob', self._h, 2 * h, n_dim, int(gof.shape[2]), gof.data_ptr(),
                               self._ptr(status), self._ptr(inside), pv.ctypes.data_as(i32), pr.ctypes.data_as(i32), len(pv),
                               md.ctypes.data_as(i32), mc.ctypes.data_as(C.POINTER(C.c_double)), prop.data_ptr(),
                               self._ptr(lp_prop))

    def mcmc_log_prob_ar1(self, gof, lag, pairs, m_dim, m_const, phi_dim, phi_const, prop, lp_prop, status=None, inside=None):
        """``mcmc_log_prob`` with the AR(1) error model of ``simplyp_amd.residuals`` (``simplyp_mcmc_log_prob_ar1``).  lag
        [4, 6, n_reaches, h] as ``Engine.gof_lag`` returns it; phi_dim [6]: the row of ``prop`` holding the variable's ``phi`` or
        -1 for ``phi_const[v]`` (0 = independent errors); the rest as for ``mcmc_log_prob``."""
        n_dim, h = (int(x) for x in prop.shape)
        pv = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        pr = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        md = np.ascontiguousarray(m_dim, dtype=np.int32)
        mc = np.ascontiguousarray(m_const, dtype=np.float64)
        pd = np.ascontiguousarray(phi_dim, dtype=np.int32)
        pc = np.ascontiguousarray(phi_const, dtype=np.float64)
        NV = len(abi.GOF_VARS)
        if md.shape != (NV,) or mc.shape != (NV,) or pd.shape != (NV,) or pc.shape != (NV,):
            raise ValueError("m_dim, m_const, phi_dim and phi_const need one entry per variable of abi.GOF_VARS")
        if gof.dim() != 4 or tuple(gof.shape[:2]) != (len(abi.GOF_STATS), NV) or int(gof.shape[3]) != h or not gof.is_contiguous():
            raise ValueError("gof %s does not match prop %s" % (tuple(gof.shape), tuple(prop.shape)))
        if tuple(lag.shape) != (len(abi.LAG_STATS),) + tuple(gof.shape[1:]) or not lag.is_contiguous():
            raise ValueError("lag %s does not match gof %s" % (tuple(lag.shape), tuple(gof.shape)))
        i32, dbl = C.POINTER(C.c_int32), C.POINTER(C.c_double)
        return self._info_call(abi.McmcInfo, 'simplyp_mcmc_log_prob_ar1', self._h, 2 * h, n_dim, int(gof.shape[2]), gof.data_ptr(),
                               lag.data_ptr(), self._ptr(status), self._ptr(inside), pv.ctypes.data_as(i32), pr.ctypes.data_as(i32),
                               len(pv), md.ctypes.data_as(i32), mc.ctypes.data_as(dbl), pd.ctypes.data_as(i32),
                               pc.ctypes.data_as(dbl), prop.data_ptr(), self._ptr(lp_prop))

    def mcmc_accept(self, theta, lp, n_accept, half, t, prop, inside, lp_prop, chain_row=None, a=2.0, seed=0):
        """The decisions of half ``half`` at step ``t``, in place on theta [n_dim, W], lp [W] and n_accept [W] (int32)
        (``simplyp_mcmc_accept``); lp_prop [W/2]: ln p of the proposals, from ``mcmc_log_prob`` or the caller's own; chain_row
        [n_dim + 1, W] or None receives the half's positions and lp after the decision."""
        n_dim, W = (int(x) for x in theta.shape)
        return self._info_call(abi.McmcInfo, 'simplyp_mcmc_accept', self._h, W, n_dim, int(half), float(a),
                               C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), C.c_uint32(int(t) & 0xFFFFFFFF),
                               self._ptr(prop), self._ptr(inside), self._ptr(lp_prop), theta.data_ptr(), self._ptr(lp),
                               self._ptr(n_accept), self._ptr(chain_row))

    # ---- multi-start Nelder-Mead (simplyp_nm_*; simplyp_amd.neldermead restates it) ----
    def nm_propose(self, sim, istate, lo, hi, target, prop, inside, member_params=None, f_tdp=None):
        """The points of every simplex's four slots (``simplyp_nm_propose``).  sim [n_dim + 1, n_dim, S] float64 and istate
        [abi.NM_N_ISTATE, S] int32 device tensors (read); lo / hi [n_dim] the box and target [n_dim] (as for ``mcmc_propose``) on
        the host; prop [n_dim, 4 S] float64, inside [4 S] int32, member_params [NP_M, 4 S] and f_tdp [4 S] device tensors that are
        written.  The library checks the values; the tensors' shapes are the caller's.  Returns the info dict."""
        n_dim, S = int(sim.shape[1]), int(sim.shape[2])
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        tg = np.ascontiguousarray(target, dtype=np.int32)
        if int(sim.shape[0]) != n_dim + 1 or lo.shape != (n_dim,) or hi.shape != (n_dim,) or tg.shape != (n_dim,):
            raise ValueError("sim must be [n_dim + 1, n_dim, S]; lo, hi and target need one entry per dimension")
        dbl = C.POINTER(C.c_double)
        return self._info_call(abi.NmInfo, 'simplyp_nm_propose', self._h, S, n_dim, lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl),
                               tg.ctypes.data_as(C.POINTER(C.c_int32)), sim.data_ptr(), self._ptr(istate), self._ptr(prop),
                               self._ptr(inside), self._ptr(member_params), self._ptr(f_tdp))

    def nm_update(self, sim, fsim, istate, prop, inside, lp_prop, max_iter, xatol=1e-4, fatol=1e-4, history=None):
        """One run's values applied in place to sim [n_dim + 1, n_dim, S], fsim [n_dim + 1, S] and istate (``simplyp_nm_update``);
        lp_prop [4 S]: ln p of the run points, from ``mcmc_log_prob`` or the caller's own; history [rows, S] or None receives the
        best value of every iteration that completes."""
        n_dim, S = int(sim.shape[1]), int(sim.shape[2])
        if int(sim.shape[0]) != n_dim + 1:
            raise ValueError("sim must be [n_dim + 1, n_dim, S]")
        return self._info_call(abi.NmInfo, 'simplyp_nm_update', self._h, S, n_dim, int(max_iter), float(xatol), float(fatol), self._ptr(prop),
                               self._ptr(inside), self._ptr(lp_prop), sim.data_ptr(), self._ptr(fsim), self._ptr(istate),
                               self._ptr(history), 0 if history is None else int(history.shape[0]))

    # ---- NSGA-II (simplyp_nsga2_*, include/simplyp_nsga2.h; simplyp_amd.nsga2 states the rule) ----
    @staticmethod
    def _box_args(n_dim, lo, hi, target):
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        tg = np.ascontiguousarray(target, dtype=np.int32)
        if lo.shape != (n_dim,) or hi.shape != (n_dim,) or tg.shape != (n_dim,):
            raise ValueError("lo, hi and target need one entry per dimension")
        dbl = C.POINTER(C.c_double)
        return (lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), tg.ctypes.data_as(C.POINTER(C.c_int32))), (lo, hi, tg)

    def nsga2_init(self, theta, lo, hi, target, member_params=None, f_tdp=None, seed=0):
        """The initial population into theta [n_dim, N] (float64 device tensor, written) and its scatter into member_params
        [NP_M, N] / f_tdp [N] (``simplyp_nsga2_init``).  lo / hi / target [n_dim] on the host, as for ``mcmc_propose``.  The
        library checks the values; the tensors' shapes are the caller's.  Returns the info dict."""
        n_dim, N = (int(x) for x in theta.shape)
        ptrs, keep = self._box_args(n_dim, lo, hi, target)
        info = self._info_call(abi.McmcInfo, 'simplyp_nsga2_init', self._h, N, n_dim, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                               *ptrs, theta.data_ptr(), self._ptr(member_params), self._ptr(f_tdp))
        del keep
        return info

    def nsga2_crowding(self, obj, sense, rank, crowd=None):
        """The crowding distance of every member within its front (``simplyp_nsga2_crowding``).  obj: contiguous float64 device
        tensor [M, n]; sense: M values +1 / -1; rank [n] int32 device tensor as ``pareto`` returns it (< 0: crowding 0).
        Returns (crowd [n] float64 device tensor, info dict)."""
        torch = self.torch
        if not torch.is_tensor(obj) or obj.dtype != torch.float64 or not obj.is_contiguous() or obj.dim() != 2 or obj.device != self.tdev:
            raise ValueError("obj must be a contiguous float64 tensor [M, n] on %s" % (self.tdev,))
        M, n = (int(x) for x in obj.shape)
        sa = np.ascontiguousarray(np.atleast_1d(np.asarray(sense)).astype(np.int32))
        if sa.shape != (M,):
            raise ValueError("sense must have one entry per objective")
        if rank.dtype != torch.int32 or tuple(rank.shape) != (n,) or not rank.is_contiguous():
            raise ValueError("rank must be a contiguous int32 tensor with one entry per member")
        if crowd is None:
            crowd = torch.empty((n,), dtype=torch.float64, device=self.tdev)
        info = self._info_call(abi.ParetoInfo, 'simplyp_nsga2_crowding', self._h, n, M, obj.data_ptr(),
                               sa.ctypes.data_as(C.POINTER(C.c_int32)), rank.data_ptr(), crowd.data_ptr())
        return crowd, info

    def nsga2_select(self, N, rank, crowd, rows=None, rows_out=None, rank_out=None, crowd_out=None):
        """Environmental selection of a set of n members down to N (``simplyp_nsga2_select``).  rank [n] int32, crowd [n] float64
        device tensors; rows: None or a contiguous float64 device tensor [n_rows, n] whose survivors' columns are gathered into
        rows_out [n_rows, N].  Returns dict(position [n], survivor [N] int32, rank [N], crowd [N], rows [n_rows, N] or None) of
        device tensors, sorted best first, plus the info fields."""
        torch = self.torch
        n, N = int(rank.shape[0]), int(N)
        if rank.dtype != torch.int32 or crowd.dtype != torch.float64 or tuple(crowd.shape) != (n,) or not rank.is_contiguous() \
                or not crowd.is_contiguous():
            raise ValueError("rank must be int32 [n] and crowd float64 [n], contiguous")
        n_rows = 0
        if rows is not None:
            if rows.dtype != torch.float64 or rows.dim() != 2 or int(rows.shape[1]) != n or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous float64 tensor [n_rows, n]")
            n_rows = int(rows.shape[0])
            if rows_out is None:
                rows_out = torch.empty((n_rows, max(N, 0)), dtype=torch.float64, device=self.tdev)
        i32 = dict(dtype=torch.int32, device=self.tdev)
        position, survivor = torch.empty((n,), **i32), torch.empty((max(N, 0),), **i32)
        rank_out = torch.empty((max(N, 0),), **i32) if rank_out is None else rank_out
        crowd_out = torch.empty((max(N, 0),), dtype=torch.float64, device=self.tdev) if crowd_out is None else crowd_out
        info = self._info_call(abi.ParetoInfo, 'simplyp_nsga2_select', self._h, n, N, rank.data_ptr(), crowd.data_ptr(),
                               position.data_ptr(), survivor.data_ptr(), n_rows, self._ptr(rows), self._ptr(rows_out),
                               rank_out.data_ptr(), crowd_out.data_ptr())
        return dict(info, position=position, survivor=survivor, rank=rank_out, crowd=crowd_out, rows=rows_out)

    def nsga2_offspring(self, theta, rank, crowd, t, lo, hi, target, child, parents=None, member_params=None, f_tdp=None,
                        k_c=4, k_m=4, p_cross=0.9, p_mut=None, seed=0):
        """The children of generation ``t`` from parents theta [n_dim, N] with rank [N] int32 and crowd [N] float64, into child
        [n_dim, N], parents [2, N] int32 (or None) and member_params / f_tdp (``simplyp_nsga2_offspring``).  k_c, k_m: the
        distribution indices are ``2^k - 1``; p_mut None = 1 / n_dim.  Returns the info dict (``n_accepted``: the pairs that crossed)."""
        n_dim, N = (int(x) for x in theta.shape)
        ptrs, keep = self._box_args(n_dim, lo, hi, target)
        p_mut = 1.0 / n_dim if p_mut is None else float(p_mut)
        info = self._info_call(abi.McmcInfo, 'simplyp_nsga2_offspring', self._h, N, n_dim, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                               C.c_uint32(int(t) & 0xFFFFFFFF), int(k_c), int(k_m), float(p_cross), p_mut, *ptrs, theta.data_ptr(),
                               self._ptr(rank), self._ptr(crowd), self._ptr(child), self._ptr(parents), self._ptr(member_params),
                               self._ptr(f_tdp))
        del keep
        return info


    # ---- Sobol' sensitivity indices (simplyp_sobol_*; simplyp_amd.sobol restates them) ----
    def sobol_design(self, N, lo, hi, target, member_params=None, f_tdp=None, seed=0, unit=None, x=None):
        """Saltelli's design of ``E = N (n_dim + 2)`` members on the device (``simplyp_sobol_design``): lo / hi [n_dim] the box and
        target [n_dim] (as for ``mcmc_propose``) on the host; member_params [NP_M, E] and f_tdp [E] float64 device tensors that
        receive the rows the targets name (the others are not touched); unit: [2, n_dim, N] unit points in [0, 1) (numpy or device
        tensor) or None for the Philox stream of ``seed``.  The library checks the values; the tensors' shapes are the caller's.
        Returns (x [n_dim, E] device tensor, info)."""
        torch = self.torch
        lo = np.ascontiguousarray(lo, dtype=np.float64)
        hi = np.ascontiguousarray(hi, dtype=np.float64)
        tg = np.ascontiguousarray(target, dtype=np.int32)
        n_dim, N = int(lo.shape[0]) if lo.ndim == 1 else -1, int(N)
        if lo.ndim != 1 or hi.shape != lo.shape or tg.shape != lo.shape:
            raise ValueError("lo, hi and target need one entry per dimension")
        E = max(N, 0) * (n_dim + 2)
        un = None
        if unit is not None:
            un = self.to_device(unit, torch.float64)
            if tuple(un.shape) != (2, n_dim, N):
                raise ValueError("unit must have shape [2, n_dim, N] = %s, got %s" % ((2, n_dim, N), tuple(un.shape)))
        if x is None:
            x = torch.empty((n_dim, E), dtype=torch.float64, device=self.tdev)
        dbl = C.POINTER(C.c_double)
        info = self._info_call(abi.SobolInfo, 'simplyp_sobol_design', self._h, N, n_dim, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                               lo.ctypes.data_as(dbl), hi.ctypes.data_as(dbl), tg.ctypes.data_as(C.POINTER(C.c_int32)),
                               self._ptr(un), x.data_ptr(), self._ptr(member_params), self._ptr(f_tdp))
        return x, info

    def sobol_indices(self, table, N, n_dim, status=None, n_boot=0, seed=0):
        """First- and total-order Sobol' indices of every row of ``table`` with ``n_boot`` bootstrap resamples
        (``simplyp_sobol_indices``); the table is only read.

        table: contiguous float64 device tensor whose LAST axis is the member axis of a design of ``N`` base samples in ``n_dim``
        dimensions, ``E = N (n_dim + 2)`` (a run's period sums, a goodness-of-fit table); status: the run's int32 device tensor
        [E] or None -- a sample with a member flagged ``abi.STATUS_NONFINITE`` takes part in nothing.
        Returns (indices, sums, n_used, info): device tensors ``(2, n_dim) + table.shape[:-1] + (1 + n_boot,)`` -- plane 0 S1, plane
        1 ST, resample 0 the point estimate --, ``(1 + n_boot,) + table.shape[:-1] + (2 n_dim + 2,)`` in the order P, S, G_0.., T_0..,
        and int32 ``[1 + n_boot]``.  ``quantiles`` on ``indices[..., 1:].contiguous()`` selects the percentile interval."""
        torch = self.torch
        E, lead, n_rows = self._member_table(table)
        N, n_dim, n_boot = int(N), int(n_dim), int(n_boot)
        if E != N * (n_dim + 2):
            raise ValueError("the table's member axis has %d entries, not N (n_dim + 2) = %d" % (E, N * (n_dim + 2)))
        if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (E,)
                                   or not status.is_contiguous()):
            raise ValueError("status must be a contiguous int32 device tensor with one entry per member")
        B = 1 + max(n_boot, 0)
        ind = torch.empty((2, max(n_dim, 0)) + lead + (B,), dtype=torch.float64, device=self.tdev)
        sums = torch.empty((B,) + lead + (2 * max(n_dim, 0) + 2,), dtype=torch.float64, device=self.tdev)
        n_used = torch.zeros((B,), dtype=torch.int32, device=self.tdev)
        info = self._info_call(abi.SobolInfo, 'simplyp_sobol_indices', self._h, N, n_dim, n_rows, table.data_ptr(), self._ptr(status),
                               n_boot, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), sums.data_ptr(), n_used.data_ptr(), ind.data_ptr())
        return ind, sums, n_used, info


    # ---- the particle filter's steps (simplyp_pf_*, simplyp_gather_members; simplyp_amd.particle restates them) ----
    def _pf_vector(self, t, E, dtype, what):
        if not self.torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (E,) or not t.is_contiguous() or t.device != self.tdev:
            raise ValueError("%s must be a contiguous %s tensor [%d] on %s" % (what, dtype, E, self.tdev))
        return t

    def pf_loglik(self, out, out_mask, obs, pairs, err_m, lw, f_tdp, reach_params, out_reaches=None, member_of_slot=None,
                  status=None, inc=None, accumulate=True):
        """Every particle's log-likelihood of the observations of the window whose daily table ``out`` [n_cols, D, n_reaches, E] a
        ``run`` left on the device (``simplyp_pf_loglik``).  obs [n_reaches, 6, D] host array, NaN = no observation; pairs: list of
        (variable index in ``abi.GOF_VARS``, position among the output reaches); err_m [n_pairs, E] float64 device tensor (member
        order); lw [E] float64 device tensor: ``lw += inc`` with ``accumulate``, ``lw = inc`` without; status [E] int32 or None;
        inc [E] float64 device tensor or None: receives the increment.  Returns the info dict."""
        torch = self.torch
        head, rp, (D, n_or, E), keep = self._daily_table(out, out_mask, reach_params, out_reaches, member_of_slot, True)
        obs = np.ascontiguousarray(obs, dtype=np.float64)
        if obs.shape != (n_or, len(abi.GOF_VARS), D):
            raise ValueError("obs must have shape %s, got %s" % ((n_or, len(abi.GOF_VARS), D), obs.shape))
        pv = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        pr = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        ft = self._f_tdp(f_tdp, E)
        if not torch.is_tensor(err_m) or err_m.dtype != torch.float64 or tuple(err_m.shape) != (len(pv), E) or not err_m.is_contiguous():
            raise ValueError("err_m must be a contiguous float64 device tensor [n_pairs, E]")
        self._pf_vector(lw, E, torch.float64, 'lw')
        if inc is not None:
            self._pf_vector(inc, E, torch.float64, 'inc')
        if status is not None:
            self._pf_vector(status, E, torch.int32, 'status')
        i32 = C.POINTER(C.c_int32)
        info = self._info_call(abi.PfInfo, 'simplyp_pf_loglik', *(head + (ft.data_ptr(), rp.data_ptr(), obs.ctypes.data_as(C.POINTER(C.c_double)),
                               pv.ctypes.data_as(i32), pr.ctypes.data_as(i32), len(pv), err_m.data_ptr(), self._ptr(status),
                               lw.data_ptr(), self._ptr(inc), 1 if accumulate else 0)))
        del keep
        return info

    def pf_weights(self, lw, w=None, q=None):
        """Normalised weights of the log weights lw [E] (``simplyp_pf_weights``).  Returns (w [E] float64, q [E] int64 -- the
        library's uint64, below 2^41 --, info with lw_max, sum_w, sum_w2, T, n_alive, n_nan)."""
        torch = self.torch
        E = int(lw.shape[0]) if torch.is_tensor(lw) and lw.dim() == 1 else -1
        self._pf_vector(lw, E, torch.float64, 'lw')
        w = torch.empty((E,), dtype=torch.float64, device=self.tdev) if w is None else self._pf_vector(w, E, torch.float64, 'w')
        q = torch.empty((E,), dtype=torch.int64, device=self.tdev) if q is None else self._pf_vector(q, E, torch.int64, 'q')
        info = self._info_call(abi.PfInfo, 'simplyp_pf_weights', self._h, E, lw.data_ptr(), w.data_ptr(), q.data_ptr())
        return w, q, info

    def pf_resample(self, q, seed, t, ancestors=None, offspring=True):
        """Systematic resampling of the integer weights q [E] (int64 device tensor) at absolute assimilation step ``t``
        (``simplyp_pf_resample``).  Returns (ancestors [E] int32, offspring [E] int32 or None, info with T and n_unique)."""
        torch = self.torch
        E = int(q.shape[0]) if torch.is_tensor(q) and q.dim() == 1 else -1
        self._pf_vector(q, E, torch.int64, 'q')
        anc = torch.empty((E,), dtype=torch.int32, device=self.tdev) if ancestors is None else self._pf_vector(ancestors, E, torch.int32, 'ancestors')
        if offspring is True:
            offspring = torch.empty((E,), dtype=torch.int32, device=self.tdev)
        elif offspring is False:
            offspring = None
        if offspring is not None:
            self._pf_vector(offspring, E, torch.int32, 'offspring')
        info = self._info_call(abi.PfInfo, 'simplyp_pf_resample', self._h, E, q.data_ptr(), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                               C.c_uint32(int(t) & 0xFFFFFFFF), anc.data_ptr(), self._ptr(offspring))
        return anc, offspring, info

    def gather_members(self, src, ancestors, dst=None):
        """``dst[..., k] = src[..., ancestors[k]]`` for a contiguous device tensor of 8-byte elements whose LAST axis is the member
        axis (``simplyp_gather_members``): the model state, member_params, reach_params, f_tdp, positions.  Out of place.
        Returns (dst, info with n_bad)."""
        torch = self.torch
        if not torch.is_tensor(src) or src.element_size() != 8 or not src.is_contiguous() or src.dim() < 1 or src.device != self.tdev:
            raise ValueError("src must be a contiguous device tensor of 8-byte elements whose last axis is the member axis")
        E = int(src.shape[-1])
        self._pf_vector(ancestors, E, torch.int32, 'ancestors')
        if dst is None:
            dst = torch.empty_like(src)
        elif not torch.is_tensor(dst) or dst.shape != src.shape or dst.dtype != src.dtype or not dst.is_contiguous() or dst.device != self.tdev:
            raise ValueError("dst must be a contiguous tensor shaped and typed like src")
        n_rows = src.numel() // E if E else 0
        info = self._info_call(abi.PfInfo, 'simplyp_gather_members', self._h, E, C.c_int64(n_rows), ancestors.data_ptr(), src.data_ptr(),
                               dst.data_ptr())
        return dst, info

    def pf_jitter(self, theta, t, a, centre, scale, lo, hi, target, member_params=None, f_tdp=None, seed=0):
        """The rejuvenation move of step ``t`` in place on theta [n_dim, E] (``simplyp_pf_jitter``): a, centre / scale / lo / hi
        [n_dim] and target [n_dim] (as for ``mcmc_propose``) on the host; member_params [NP_M, E] and f_tdp [E] device tensors
        receive the rows the targets name.  Returns the info dict (n_outside)."""
        n_dim, E = (int(x) for x in theta.shape)
        arrs = [np.ascontiguousarray(x, dtype=np.float64) for x in (centre, scale, lo, hi)]
        tg = np.ascontiguousarray(target, dtype=np.int32)
        if any(x.shape != (n_dim,) for x in arrs) or tg.shape != (n_dim,):
            raise ValueError("centre, scale, lo, hi and target need one entry per dimension")
        dbl = C.POINTER(C.c_double)
        return self._info_call(abi.PfInfo, 'simplyp_pf_jitter', self._h, E, n_dim, C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                               C.c_uint32(int(t) & 0xFFFFFFFF), float(a), *([x.ctypes.data_as(dbl) for x in arrs]
                               + [tg.ctypes.data_as(C.POINTER(C.c_int32)), theta.data_ptr(), self._ptr(member_params), self._ptr(f_tdp)]))


def interpolate_quantiles(lower, upper, q, n_used):
    """numpy's ``method='linear'`` quantile from the two order statistics ``Engine.quantiles`` returns (host arrays
    [K, ...]): h = q (n - 1) formed exactly as the library forms it, gamma = h - floor(h), and numpy's own lerp --
    ``lo + (hi - lo) gamma`` for gamma < 0.5, ``hi - (hi - lo) (1 - gamma)`` otherwise."""
    lower = np.asarray(lower, dtype=np.float64)
    upper = np.asarray(upper, dtype=np.float64)
    qa = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if int(n_used) < 1:
        return np.full(lower.shape, np.nan)
    h = qa * np.float64(int(n_used) - 1)
    gamma = (h - np.floor(h)).reshape((-1,) + (1,) * (lower.ndim - 1))
    diff = upper - lower
    with np.errstate(invalid='ignore'):
        data = np.where(gamma >= 0.5, upper - diff * (1 - gamma), lower + diff * gamma)
    return data


def interpolate_time_quantiles(lower, upper, q, n_days):
    """numpy's ``method='linear'`` quantile from the two order statistics ``Engine.time_quantiles`` returns (host arrays
    [K, n_series, P, ...]) with a day count per period (``info['n_days']`` [P]): ``interpolate_quantiles`` -- the same h,
    gamma and lerp -- period by period; NaN where a period holds no day."""
    lower = np.asarray(lower, dtype=np.float64)
    upper = np.asarray(upper, dtype=np.float64)
    n_days = np.atleast_1d(np.asarray(n_days))
    if lower.ndim < 3 or lower.shape[2] != len(n_days):
        raise ValueError("lower / upper must be [K, n_series, P, ...] with P = len(n_days)")
    data = np.empty(lower.shape, dtype=np.float64)
    for p, n in enumerate(n_days):
        data[:, :, p] = interpolate_quantiles(lower[:, :, p], upper[:, :, p], q, int(n))
    return data


_engines = {}


def get_engine(device=0, replica=0):
    """Process-wide engine per device (contexts hold grow-only device scratch).  ``replica`` > 0 gives a further context on the
    same device (contexts are not re-entrant: two host threads that drive one GPU need one each)."""
    key = (int(device), int(replica))
    if key not in _engines:
        _engines[key] = Engine(device)
    return _engines[key]
