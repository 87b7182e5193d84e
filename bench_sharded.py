"""bench.py --config 5: the 100M-point target cut into kd slabs + halo over the ranks.

Every rank indexes its slab of the target plus the halo (pcl_amd.dist.ShardedTarget), holds the whole source,
serves the source points whose current position lies in its region, and takes part in the per-iteration
ncclAllReduce of the 32-double record.  `--replicated` runs the comparison point of the survey: the whole target
indexed on every rank, the source cut into slabs.  Either way the job registers the same two clouds, so `value`
(correspondences of the whole job per second) is comparable; the run is strong scaling in the number of GPUs.
"""
import os
import time

import numpy as np

B_ALG_SEARCH = 40.0
HBM_PEAK_GBS = 8000.0


def cpu_baseline_config5(args, n, src_dev, max_dist):
    """The oracle on the host cores against the WHOLE n-point target (regenerated on the device, downloaded once): kd-tree,
    k normals, then ONE point-to-plane iteration of a bounded sample of the source (the first 5M points) on all threads --
    N = 1 only, ~1 minute at 100M points, most of it the single-threaded tree build (as in FLANN)."""
    import time
    from pcl_amd import synth
    from oracle import pcl_oracle as orc
    import bench
    cores = orc.default_threads()
    tgt_h = synth.gaussian_surface_device(n, synth.TARGET_SEED).cpu().numpy()
    t0 = time.perf_counter()
    tree = orc.KdTree(tgt_h)
    build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    nrm, _ = tree.normals(tgt_h, args.knn, viewpoint=(0, 0, 10), nthreads=cores)
    normals_s = time.perf_counter() - t0
    m = min(n, 5_000_000)
    sample = src_dev[:m].cpu().numpy()
    r = orc.icp_align(tree, tgt_h, sample, mode=1, tgt_normals=nrm, max_iterations=1, nthreads=cores,
                      max_correspondence_distance=max_dist, transformation_epsilon=0.0)
    it = max(r["iterations"], 1)
    per_iter = r["seconds_total"] / it
    return {"value": round(r["num_correspondences"] / per_iter, 1), "unit": "correspondences/s", "cores": cores,
            "threads_used": cores, "host_hardware_threads": bench.host_cpus()[0], "host_physical_cores": bench.host_cpus()[1],
            "kind": "port",
            "note": "a dependency-free RESTATEMENT of PCL's CPU path (oracle/pcl_oracle.c), not PCL + FLANN: a stated baseline, "
                    "never a target (roofline.frac is the measure of the kernel)",
            "sample": "the whole %d-point target indexed (kd-tree build %.1f s single-thread, k=%d normals %.1f s on %d threads), "
                      "ONE ICP iteration of the first %d source points on %d threads (search %.3f s)" %
                      (n, build_s, args.knn, normals_s, cores, m, cores, r["seconds_search"] / it),
            "ms_per_iteration_of_sample": round(per_iter * 1e3, 2)}


def run_config5(args, ctx, comm, rank, local_rank, world, fence):
    import torch
    import torch.distributed as dist
    import pcl_amd
    from pcl_amd import synth
    from pcl_amd.dist import ShardedTarget, shard_range

    n = args.points or 100_000_000
    max_dist = 0.1
    # The clouds are generated where they are used -- in device memory (pcl_amd.synth.gaussian_surface_device: the same
    # counter-based stream) -- and cut there too (pclhip_partition_slabs / pclhip_select_region on a device cloud:
    # shard_dev.hip): no rank holds the whole target on the host.
    dev = torch.device("cuda", torch.cuda.current_device())
    t0 = time.perf_counter()
    tgt = synth.gaussian_surface_device(n, synth.TARGET_SEED, device=dev)
    torch.cuda.synchronize()
    gen_s = time.perf_counter() - t0
    T_inv = np.linalg.inv(synth.ground_truth_transform())
    setup = {}
    if args.replicated:
        start, count = shard_range(n, rank, world)
        src = synth.apply_rigid_device(T_inv, synth.gaussian_surface_device(count, synth.SOURCE_SEED, start=start, device=dev))
        tree = pcl_amd.KdTree(ctx)
        tree.setInputCloud(tgt)
        ne = pcl_amd.NormalEstimation(ctx)
        ne.setInputCloud(tgt)
        ne.setSearchMethod(tree)
        ne.setKSearch(args.knn)
        ne.setViewPoint(0, 0, 10)
        ne.compute(want_output=False)
        region = None
        setup.update(index_points=tree.size(), index_build_ms=round(tree.build_ms(), 3), normals_kernel_ms=round(tree.lastKernelMs(), 3))
    else:
        src = synth.apply_rigid_device(T_inv, synth.gaussian_surface_device(n, synth.SOURCE_SEED, device=dev))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        # --virtual-world G --virtual-rank r on one GPU: this process plays rank r of G (slab, halo and region of that
        # rank; the record is not exchanged, so the alignment is the one of the points this rank serves -- what is
        # measured is a rank's work per iteration, e.g. with and without the served-group lists, --full-pass)
        vworld = args.virtual_world if (args.virtual_world > 1 and world == 1) else 0
        if getattr(args, "full_pass", False):
            ctx.setOption("served_groups", 0)
        st = ShardedTarget(ctx, tgt, args.virtual_rank if vworld else rank, vworld or world, max_dist, k_normals=args.knn,
                           viewpoint=(0, 0, 10))
        tree, region = st.tree, st.region
        from pcl_amd.dist import select_region
        owned_points = int(len(select_region(tgt, st.region, 0.0)))
        setup.update(index_points=tree.size(), owned_points=owned_points, halo_margin=round(st.margin, 5),
                     kth_neighbour_distance=round(st.kth, 6),
                     normals_exact=bool(st.normals_exact), index_build_ms=round(tree.build_ms(), 3),
                     shard_setup_s=round(time.perf_counter() - t1, 2), shard_setup_stages_s=st.timings)
    del tgt
    icp = pcl_amd.IterativeClosestPointWithNormals(ctx)
    icp.setSearchMethodTarget(tree, True)
    icp.setInputSource(src)
    icp.setMaximumIterations(20)
    icp.setMaxCorrespondenceDistance(max_dist)
    icp.setTransformationEpsilon(1e-10)
    from pcl_amd.dist import attach_collective
    attach_collective(icp, comm, local_rank, world)
    if region is not None:
        icp.setRegion(region)
    from pcl_amd.dist import timed_steps
    steps, elapsed = timed_steps(icp, args.steps, args.warmup, fence, world)
    # ---- self-validation (VERDICT r2 #7c): what every rank served in the last timed iteration, gathered over the job.
    # The served sets partition the source (every point has exactly one owner), so their sizes must add up to the
    # all-reduced count the step records carry -- an N > 1 line that fails this is not a measurement.
    served = len(icp.fetchCorrespondences()[0])
    mine = {"rank": rank, "served": int(served), "index_points": int(tree.size()),
            "halo_points": None if args.replicated else int(tree.size()) - int(setup.get("owned_points", 0))}
    if world > 1:
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
    else:
        gathered = [mine]
    total_served = sum(g["served"] for g in gathered)
    last_count = int(steps[-1]["num_correspondences"])
    # (the loop queues one launch ahead of the records it hands back: the match arrays may belong to the step after the
    # last record, so the sum is compared with the counts of the run's steps, not only with the last one)
    if total_served not in {int(s["num_correspondences"]) for s in steps}:
        raise SystemExit("config 5 self-check failed: the ranks served %d pairs, the all-reduced records say %s"
                         % (total_served, sorted({int(s["num_correspondences"]) for s in steps})))
    if rank != 0:
        return None
    cpu = None
    if world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline_config5(args, n, src, max_dist)
    ncorr = float(sum(s["num_correspondences"] for s in steps))       # all-reduced: the whole job's count
    search_ms = sum(s["search_ms"] for s in steps)
    avg_kernel_s = search_ms / max(args.steps, 1) / 1e3
    achieved = B_ALG_SEARCH * (ncorr / max(args.steps, 1) / world) / avg_kernel_s / 1e9
    return {
        "metric": "ICP correspondences/sec", "value": round(ncorr / elapsed, 1), "unit": "correspondences/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / max(args.steps, 1) * 1e3, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32 search / f64 accumulate",
        "data": "synthetic",
        "config": {"workload": "config 5: %d-point synthetic Gaussian-surface target and source, k=%d normals + point-to-plane "
                               "ICP, max_dist %.2f; %s" %
                               (n, args.knn, max_dist,
                                "target replicated, source cut into %d slabs" % world if args.replicated else
                                "target cut into %d kd slabs + halo, source replicated and routed by current position%s" %
                                (getattr(args, "virtual_world", 0) if (getattr(args, "virtual_world", 0) > 1 and world == 1) else world,
                                 "; ONE GPU playing rank %d of that job, no collective" % args.virtual_rank
                                 if (getattr(args, "virtual_world", 0) > 1 and world == 1) else "")),
                   "target_points": n, "source_points": n,
                   "parallelism": ("source slabs x%d" if args.replicated else "target kd slabs + halo x%d") % world +
                                  ", ncclAllReduce of the 32-double record per iteration"},
        "roofline": {"bound": "hbm", "kernel": "icp_search_kernel", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None,
                     "alg_bytes_per_corr": B_ALG_SEARCH, "avg_kernel_ms": round(avg_kernel_s * 1e3, 4),
                     "note": "rank 0's launches; achieved counts the correspondences rank 0 serves on average"},
        "cpu_baseline": cpu,
        "per_step": [{"iteration": s["iteration"], "search_ms": round(s["search_ms"], 4), "step_ms": round(s["step_ms"], 4),
                      "ended": s["alignment_ended"], "state": s["state"]} for s in steps],
        "setup": dict(setup, synth_gen_s=round(gen_s, 1)),
        "virtual_rank": ({"world": args.virtual_world, "rank": args.virtual_rank,
                          "served_groups_lists": not getattr(args, "full_pass", False),
                          "note": "value / ms_per_step are ONE rank's share of the job; not a multi-GPU measurement"}
                         if (args.virtual_world > 1 and world == 1) else None),
        "self_check": {"rccl_nranks": world if comm is not None else 1, "native_communicator": comm is not None,
                       "served_sum_equals_allreduced_count": True, "allreduced_count_last_step": last_count,
                       "per_rank": gathered},
    }
