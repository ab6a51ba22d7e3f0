"""What `bench.py --gpus N` adds to its line when N > 1, beside `value` (the eager loop over torch.distributed P2P, the safe
default): a table that proves N RCCL ranks on N devices, and a GUARDED section that takes the decomposed step through the paths
round 5 built -- the library's own RCCL transport checked against torch's ghosts between the real ranks, whole check periods
replayed from hipGraphs with the exchange inside (standin.BrickRun), the direct-store `peer` transport -- none of which has ever
run between two devices on this pool.  A failure or a hang there must cost only its own field, never the JSON line: every rank
arms the same per-phase watchdog; when one fires, rank 0 prints the line as it stands with the phase's skip reason and every rank
leaves (os._exit: no re-exec, no new process on a GPU-initialised one).

north_star: "particle-domain decomposition across the 8 GPUs of one node uses RCCL over xGMI only for the ghost-particle halo";
the exchange is what HOOMD's Communicator does for the reference (htf/TensorflowCompute.cc:143-148 reads the ghosts in place)."""
import json
import os
import sys
import threading
import time

import numpy as np
import torch


def rank_table(E):
    """Per rank: the device it computes on (uuid, PCI bus id, name), what its communicators say about themselves.  Gathered into
    the line so that a scaling run can be audited from the JSON alone."""
    dev = E.dev
    props = torch.cuda.get_device_properties(dev)
    rec = {"rank": E.rank, "local_device_index": dev.index, "device_name": props.name,
           "device_uuid": str(getattr(props, "uuid", None)),
           "pci": "%04x:%02x:%02x" % (getattr(props, "pci_domain_id", 0), getattr(props, "pci_bus_id", 0), getattr(props, "pci_device_id", 0)),
           "pid": os.getpid(), "backend": E.backend}
    if E.dist is not None:
        rec["process_group"] = {"backend": E.dist.get_backend(), "world_size": E.dist.get_world_size(), "rank": E.dist.get_rank()}
    if E.dist is None:
        return [rec]
    table = [None] * E.world
    E.dist.all_gather_object(table, rec)
    return table


def add_native_comm_info(table_entry, native):
    """ncclCommCount / UserRank / CuDevice of the library's own communicator (csrc/halo.hip)."""
    import ctypes as C
    from hoomd_tf_amd import _lib
    n, r, d = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = _lib.lib.htf_halo_comm_info(native._h, C.byref(n), C.byref(r), C.byref(d))
    table_entry["rccl_communicator"] = ({"nranks": n.value, "rank": r.value, "device": d.value} if rc == 0
                                        else {"error": _lib.lib.htf_last_error().decode(errors="replace")})
    return table_entry


class PhaseWatchdog:
    """arm(name, seconds) before a phase that may hang, disarm() behind it.  Every rank arms the same phases in the same order
    (they are in lockstep at the barrier before each), so a hang is noticed by all of them within the same second: rank 0 prints
    the line it has (``emit(reason)``), everybody exits with status 0."""

    def __init__(self, rank, emit):
        self.rank, self.emit = rank, emit
        self._gen = 0
        self._lock = threading.Lock()
        self.fired = None

    def arm(self, name, seconds):
        with self._lock:
            self._gen += 1
            gen = self._gen
        t = threading.Thread(target=self._wait, args=(gen, name, float(seconds)), daemon=True)
        t.start()

    def disarm(self):
        with self._lock:
            self._gen += 1

    def _wait(self, gen, name, seconds):
        t_end = time.monotonic() + seconds
        while time.monotonic() < t_end:
            time.sleep(0.05)
            with self._lock:
                if self._gen != gen:
                    return
        with self._lock:
            if self._gen != gen:
                return
            self._gen = -1                       # (nothing may re-arm: we are leaving)
        reason = "watchdog: phase %r did not finish within %.0f s" % (name, seconds)
        self.fired = reason
        try:
            if self.rank == 0:
                self.emit(reason)
            else:
                time.sleep(0.5)                  # (rank 0's line first)
        finally:
            sys.stdout.flush()
            sys.stderr.flush()
            os._exit(0)


def _same(a, b):
    return bool(torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)))


def _agree(E, ok):
    """Every rank learns whether EVERY rank got through the phase (a MIN all-reduce over the job's own process group)."""
    t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float32, device=E.dev if E.backend == "nccl" else "cpu")
    E.dist.all_reduce(t, op=E.dist.ReduceOp.MIN)
    return bool(t.item() > 0.5)


def _timed_replay(E, brun, steps, windows):
    """`windows` windows of `steps` replayed steps, each bracketed by barrier + synchronize, max over the ranks."""
    out = []
    for _ in range(windows):
        torch.cuda.synchronize()
        E.dist.barrier()
        t0 = time.perf_counter()
        brun.run(steps, graph=True)
        torch.cuda.synchronize()
        E.dist.barrier()
        el = time.perf_counter() - t0
        t = torch.tensor([el], dtype=torch.float64, device=E.dev if E.backend == "nccl" else "cpu")
        E.dist.all_reduce(t, op=E.dist.ReduceOp.MAX)
        out.append(float(t.item()))
    return out


def guarded_section(E, live, out, emit):
    """-> dict of fields for the line: `native_selftest`, `graph_variant`, `graph_variant_peer`, each a record or a named skip.
    ``live``: the LJ run's objects as run_md left them (sysm, nl, ctx, nve, brun, state, args, step)."""
    args, sysm, nl, brun, state = live["args"], live["sysm"], live["nl"], live["brun"], live["state"]
    dom = nl.domain
    P = nl.check_period
    limit = float(os.environ.get("HTF_BENCH_PHASE_S", "60"))
    res = {}
    wd = PhaseWatchdog(E.rank, lambda why: emit(dict(res, guarded_section_ended_by=why)))
    steps = max(args.steps, P) // P * P
    windows = max(args.windows, 1)

    def phase(name, fn, seconds=limit):
        """Run fn() on every rank under the watchdog; -> (ok on every rank, this rank's result or error text)."""
        torch.cuda.synchronize()
        E.dist.barrier()
        wd.arm(name, seconds)
        try:
            val, err = fn(), None
        except Exception as e:  # noqa: BLE001
            val, err = None, "%s: %s" % (type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        ok = _agree(E, err is None)
        wd.disarm()
        if not ok and err is None:
            err = "another rank failed in this phase"
        return ok, (val if ok else err)

    def selftest(transport, bring_up):
        """20 MD steps of the timed loop (torch transport); after each, the ghosts ``transport`` delivers against the torch transport's."""
        def fn():
            dom.exchange_end()
            bring_up()
            nat = dom._native
            cap = dom.cap
            bad = 0
            for _ in range(20):
                dom._native, dom.transport = None, "torch"
                live["step"]()                          # one MD step of the timed loop: new positions
                dom.exchange_end()
                dom.exchange()
                torch.cuda.synchronize()
                want = sysm.pos[cap:].clone()
                sysm.pos[cap:, :3] = float("nan")       # (what the exchange under test must overwrite)
                dom._native, dom.transport = (nat if transport == "native" else None), transport
                dom.exchange()
                torch.cuda.synchronize()
                bad += 0 if _same(want, sysm.pos[cap:]) else 1
            dom._native, dom.transport = None, "torch"
            if bad:
                raise RuntimeError("%d of 20 exchanges delivered other ghosts than the torch transport" % bad)
            dom._native = nat
            return {"exchanges": 20, "bit_equal_to_torch_transport": True, "messages_per_exchange": dom.n_msg}
        return fn

    def native_up():
        from hoomd_tf_amd import _lib
        if not _lib.lib.htf_halo_available():
            raise RuntimeError("librccl could not be loaded by libhtf_amd.so")
        if E.backend != "nccl" and torch.cuda.device_count() < E.world:
            raise RuntimeError("%d ranks share %d device(s) (a %s rehearsal): RCCL refuses two ranks on one device"
                               % (E.world, torch.cuda.device_count(), E.backend))
        dom._make_native()                              # collective: ncclCommInitRank on every rank

    def replay(transport):
        def fn():
            dom.exchange_end()
            dom.transport = transport
            sysm.timestep = state["ts"]
            brun._graphs = None
            brun._arr = None
            brun.run((-sysm.timestep) % P + 4 * P)                      # eager under this transport, ends on a check step
            brun.run(max(args.warmup, 4 * P) // P * P, graph=True)     # capture + warm replays
            w = _timed_replay(E, brun, steps, windows)
            state["ts"] = sysm.timestep
            torch.cuda.synchronize()
            dom.counts_host()                                           # (raises on overflow / lost-particle / halo-timeout flags)
            f = sysm.force
            if not bool(torch.isfinite(f).all()):
                raise RuntimeError("non-finite forces after the replay")
            n_now = dom.n_local
            t = torch.tensor([float(f[:, 3].double().sum()), float((sysm.vel[:, :3].double() ** 2).sum()), float(n_now)],
                             dtype=torch.float64, device=E.dev if E.backend == "nccl" else "cpu")
            E.dist.all_reduce(t)
            el = float(np.median(w))
            dom.exchange_end()
            dom.transport = "torch"                                     # (what the timed loop and the next self-test step with)
            return {"note": "whole check periods of the decomposed step (check, halo, force rows, integrate-and-pack; migration + re-plan + "
                            "list rebuild in the second graph) replayed from hipGraphs per rank, transport %r; same decisions as the eager loop" % transport,
                    "halo": {"transport": transport}, "value": steps / el, "unit": "steps/s", "steps": steps, "ms_per_step": el / steps * 1e3,
                    "windows_ms_per_step": [x / steps * 1e3 for x in w], "rebuild_cycles": brun.n_rebuild_cycles, "dangerous_builds": brun.dangerous_builds,
                    "energy_per_particle": float(t[0] / t[2]), "kT": float(t[1] / (3.0 * t[2])), "particles": int(t[2])}
        return fn

    # ---- the library's own RCCL communicator between the real ranks: its ghosts against the torch transport's, then the replay
    ok, val = phase("native-selftest", selftest("native", native_up))
    if not ok:
        dom._native, dom.transport = None, "torch"      # (the timed loop's transport stays as it was)
    res["native_selftest"] = val if ok else {"skipped": val}
    if ok:
        ok, val = phase("graph-replay-native", replay("native"), seconds=2 * limit)
        res["graph_variant"] = val if ok else {"skipped": val}
        if not ok:
            return res                                  # (a replay that failed half way leaves the ranks out of step: stop here)
    else:
        res["graph_variant"] = {"skipped": "transport 'native' is not available: " + str(val)}

    # ---- the halo, the migration messages and the distance check's all-reduce WITHOUT a library (brick.py transport "peer": stores
    # into the neighbors' memory, csrc/brick.hip *_peer_kernel + csrc/mailbox.hip): mapping, self-test, replay
    ok, val = phase("peer-selftest", selftest("peer", dom._make_peer))
    if not ok:
        dom._native, dom.transport = dom._native, "torch"
    res["peer_selftest"] = dict(val, inbox_memory=getattr(dom, "peer_memory", None)) if ok else {"skipped": val}
    if not ok:
        res["graph_variant_peer"] = {"skipped": "transport 'peer' is not available: " + str(val)}
        return res
    ok, val = phase("graph-replay-peer", replay("peer"), seconds=2 * limit)
    if ok:
        val["halo"]["inbox_memory"] = getattr(dom, "peer_memory", None)
    res["graph_variant_peer"] = val if ok else {"skipped": val}
    return res


def promote_verified(out):
    """`value` is the whole job's throughput on the fastest path that RAN TO THE END on every rank and passed its checks: the eager
    loop over torch.distributed is what is timed first (nothing in it can hang a node), the replayed decomposed step -- the path
    the library ships for production, transports `native` / `peer` -- is timed in the guarded section; when a replay timed the
    same number of steps, kept every particle, and left the system at the eager loop's temperature and energy (NVE: +-10 % / +-5 %
    between two points of one trajectory), it becomes `value` and the eager figure stays on the line as `eager`."""
    best, name = None, None
    for key in ("graph_variant", "graph_variant_peer"):
        v = out.get(key)
        if not (isinstance(v, dict) and "value" in v and v.get("steps") == out.get("steps")):
            continue
        e0, k0 = out.get("energy_per_particle"), out.get("kT_final")
        if e0 is None or k0 is None or not (np.isfinite(v["energy_per_particle"]) and np.isfinite(v["kT"])):
            continue
        if abs(v["kT"] - k0) > 0.1 * abs(k0) or abs(v["energy_per_particle"] - e0) > 0.05 * abs(e0):
            continue
        if v["value"] > out["value"] and (best is None or v["value"] > best["value"]):
            best, name = v, key
    if best is None:
        out["value_path"] = "eager loop (torch.distributed transport)"
        return out
    out["eager"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "unit": out["unit"],
                    "note": "the same steps driven from Python over the torch.distributed transport (timed first; the safe default)"}
    out["value"], out["ms_per_step"] = best["value"], best["ms_per_step"]
    if "particle_steps_per_s" in out and "global_particles" in out.get("config", {}):
        out["eager"]["particle_steps_per_s"] = out["particle_steps_per_s"]
        out["particle_steps_per_s"] = out["value"] * out["config"]["global_particles"]
    out["value_path"] = "%s: whole check periods replayed from hipGraphs per rank, transport %r" % (name, best["halo"]["transport"])
    return out
