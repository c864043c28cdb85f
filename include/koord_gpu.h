/*
 * koord_gpu.h — C-ABI of the MI355X batched Filter/Score engine for koord-scheduler.
 *
 * This is the drop-in boundary between the (Go) koord-scheduler plugins and the
 * HIP engine.  Every entry point takes plain pointers and sizes; no torch / HIP
 * types appear in the signatures (streams are passed as opaque `void*`).
 *
 * Which reference surface each entry replaces (paths relative to the reference
 * repository PeterChg/koordinator @ 2025-01-12):
 *
 *   kg_engine_create        plugin construction: loadaware.New (pkg/scheduler/plugins/loadaware/load_aware.go:76-110),
 *                           NodeResourcesFit (upstream k8s v1.24.15 noderesources.NewFit; profile
 *                           config/manager/scheduler-config.yaml:17-31)
 *   kg_build_pod_rows       PreFilter-time pod preprocessing: NodeResourcesFit computePodResourceRequest
 *                           (in-repo mirror reservation/transformer.go:316-346), estimator.EstimatePod
 *                           (loadaware/estimator/default_estimator.go:57-108), GetPodPriorityClassWithDefault
 *                           (apis/extension/priority_utils.go:26-47), isDaemonSetPod (loadaware/helper.go:189-196)
 *   kg_build_node_rows      snapshot ingest of NodeInfo + NodeMetric + podAssignCache: the node-only parts of
 *                           LoadAware.Filter (load_aware.go:123-254) and LoadAware.Score (load_aware.go:269-376),
 *                           EstimateNode (default_estimator.go:110-129)
 *   kg_snapshot_upsert      informer/event feeders: podAssignCache.OnAdd/OnUpdate/OnDelete
 *                           (loadaware/pod_assign_cache.go:82-117), upstream Cache.UpdateSnapshot
 *   kg_eval                 per-(pod,node) hot loops: framework.FilterPlugin.Filter and ScorePlugin.Score of
 *                           LoadAwareScheduling (load_aware.go:123, :269) and NodeResourcesFit (upstream
 *                           fitsRequest / LeastAllocated), plus the per-pod max of upstream selectHost
 *   kg_place                the sequential scheduling cycle (upstream scheduleOne → Filter → Score → selectHost →
 *                           Reserve) for a queue of pods, with Reserve deltas of LoadAware.Reserve
 *                           (load_aware.go:260-267) and NodeInfo.AddPod (mirror reservation/transformer.go:293-306)
 *   kg_commit               one Reserve (AssumePod + LoadAware.Reserve) of a pod on a node
 *   kg_unreserve            the plugins' Unreserve, run by the framework when Permit, PreBind or Bind fails after
 *   / kg_row_unreserve      Reserve (under Coscheduling for a whole gang at once): LoadAware podAssignCache.unAssign
 *                           (loadaware/load_aware.go:265, pod_assign_cache.go:70-80), NodeNUMAResource
 *                           resourceManager.Release → NodeAllocation.release (nodenumaresource/plugin.go:421,
 *                           node_allocation.go:105-131), Reservation forgetPod → ReservationInfo.RemoveAssignedPod
 *                           (reservation/plugin.go:552-574, frameworkext/reservation_info.go:390-401), ElasticQuota
 *                           GroupQuotaManager.UnreservePod (elasticquota/plugin.go:339-351,
 *                           core/group_quota_manager.go:799-805), and NodeInfo.RemovePod of ForgetPod
 *   kg_place_gangs          kg_place with Coscheduling's Strict-mode rejection inside the batch: a gang member without
 *   / kg_gang_plan          a node rejects its gang group (coscheduling/core/core.go:276-306, :362-388), the members
 *                           already reserved are Unreserved (:343-360) and the rest fail PreFilter (:255-269); the
 *                           verdict per gang is the caller's Permit decision (gang.go:480-495)
 *   kg_cycle_one            one pass of upstream scheduleOne for one pod in one launch: Filter + Score over every
 *                           node, selectHost, and (KG_CYCLE_COMMIT) the Reserve of the chosen node
 *   kg_candidates           upstream numFeasibleNodesToFind + prioritizeNodes over the engine's plugins: per pod the K
 *   / kg_candidates_merge   best feasible nodes of ALL nodes (not of a sampled subset) with each engine plugin's score,
 *                           the hand-over to a framework that adds Score plugins of its own
 *   kg_bound_set / _update  NodeInfo.Pods of every node as the preemption dry run reads it: the bound pods' requests, quota
 *                           group, priority (corev1helpers.PodPriority) and start time (util.GetPodStartTime)
 *   kg_preempt              ElasticQuota's PostFilter preemption (elasticquota/plugin.go:302-321): SelectVictimsOnNode
 *   / kg_row_preempt        (preempt.go:111-215) dry-run on ALL nodes (GetOffsetAndNumCandidates, preempt.go:43-45), and
 *   / kg_preempt_merge      upstream pickOneNodeForPreemption (k8s v1.24.15 framework/preemption/preemption.go)
 *   kg_pdb_thresholds       filterPodsWithPDBViolation (preempt.go:217-267) folded into one threshold per bound pod, the
 *   / kg_bound_pdb_set      engine's plane of them and the dry run's PDB form: violating victims reprieved first,
 *   / kg_row_preempt_pdb    numViolatingVictim as the pick's second criterion
 *   kg_rsv_set              reservation cache feed (reservation/cache.go:249-269 forEachAvailableReservationOnNode,
 *                           frameworkext/reservation_info.go:200-300): per-node reservation slots for the
 *                           Reservation plugin's restore / Filter / Score / Reserve (reservation/transformer.go:49-291,
 *                           plugin.go:311-476, scoring.go:42-203, nominator.go:76-135)
 *   kg_quota_set            ElasticQuota group state for its PreFilter / Reserve (elasticquota/plugin.go:210-255,
 *                           :323-337; core/group_quota_manager.go:613-650, :791-797)
 *   kg_elig_set / _update   the node-only Filter verdicts of plugins the engine does not model (NodeAffinity /
 *                           nodeSelector, TaintToleration, NodeName, NodeUnschedulable, ...) as per-class node masks
 *                           (kg_pod_row.elig_class), ANDed into feasibility wherever the engine chooses a node
 *
 * Units follow k8s Quantity conversions used by the plugins: cpu-like resources
 * (KG_RES_CPU) in milli-units (Quantity.MilliValue), every other resource in
 * base units (Quantity.Value).  batch-cpu / mid-cpu are stored as their Value()
 * (the reference encodes them in milli-cores already).
 *
 * Error model: every function returns kg_status (0 = ok, < 0 = error); the
 * message of the last error of an engine is available from kg_last_error().
 * Threading: one engine = one HIP stream; calls on one engine must be serialized
 * by the caller (the Go side holds a mutex), results are plain host memory.
 */
#ifndef KOORD_GPU_H
#define KOORD_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KG_ABI_VERSION 13
#define KG_QUOTA_MAX_DEPTH 64 /* longest kg_quota parent chain (cycles are rejected) */

/* largest kg_config.place_chunk / kg_place_chunk_resolve chunk (the resolve kernel's touched list) */
#define KG_PLACE_CHUNK_MAX 1024

/* kg_place_chunk_eval / _resolve partial buffer: KG_PARTIAL_SLOTS uint32 per (pod, 1024-node tile) —
 * the tile's best keys in descending order, 0-padded (nodes outside the fp64 fast-path bounds are not
 * listed: the resolve re-scores them from the engine's slow-node list).  Slots of a tile come from one
 * rank only, so ranks merge buffers with an element-wise max. */
#define KG_PARTIAL_SLOTS 16

/* ------------------------------------------------------------------ */
/* status codes                                                          */
/* ------------------------------------------------------------------ */
typedef int32_t kg_status;
#define KG_OK 0
#define KG_ERR_INVALID_ARG (-1)
#define KG_ERR_HIP (-2)
#define KG_ERR_UNSUPPORTED (-3)
#define KG_ERR_RANGE (-4)
#define KG_ERR_STATE (-5)
#define KG_NOT_FOUND 1       /* a search found nothing (kg_cpuset_take: no cpuset satisfies the request) */

/* upstream framework.Code values used in filter results */
#define KG_CODE_SUCCESS 0
#define KG_CODE_ERROR 1
#define KG_CODE_UNSCHEDULABLE 2
#define KG_CODE_UNSCHEDULABLE_AND_UNRESOLVABLE 3

/* ------------------------------------------------------------------ */
/* resources                                                             */
/* ------------------------------------------------------------------ */
#define KG_NUM_RES 12
#define KG_NUM_EXT_RES 5          /* named scalar slots KG_RES_EXT0 .. KG_RES_EXT4 */
#define KG_RES_NAME_MAX 64        /* bytes of a slot name in kg_config.ext_resource_names, NUL included */
enum kg_resource {
    KG_RES_CPU = 0,               /* "cpu"                         MilliValue */
    KG_RES_MEMORY = 1,            /* "memory"                      Value      */
    KG_RES_EPHEMERAL_STORAGE = 2, /* "ephemeral-storage"           Value      */
    KG_RES_BATCH_CPU = 3,         /* "kubernetes.io/batch-cpu"     Value      */
    KG_RES_BATCH_MEMORY = 4,      /* "kubernetes.io/batch-memory"  Value      */
    KG_RES_MID_CPU = 5,           /* "kubernetes.io/mid-cpu"       Value      */
    KG_RES_MID_MEMORY = 6,        /* "kubernetes.io/mid-memory"    Value      */
    /* the named scalar slots: extended resources (nvidia.com/gpu, koordinator.sh/gpu-core, koordinator.sh/rdma,
     * ...) and hugepages-<size>, named by kg_config.ext_resource_names (default: slot 0 "example.com/gpu", the
     * others unused).  Every plugin on the path treats them as the ScalarResources of framework.Resource:
     * NodeResourcesFit compares each requested one (fitsRequest), scores those its ScoringStrategy weighs,
     * LoadAware weighs those its resourceWeights name, Reservation / ElasticQuota add them up. */
    KG_RES_EXT0 = 7, KG_RES_EXT1 = 8, KG_RES_EXT2 = 9, KG_RES_EXT3 = 10, KG_RES_EXT4 = 11,
    KG_RES_EXTENDED = KG_RES_EXT0
};
/* resources that upstream schedutil.IsScalarResourceName() treats as scalar */
#define KG_SCALAR_RES_MASK 0xFF8u

/* A corev1.ResourceList restricted to the resources above: `present` is the
 * key set (bit r ⇔ key r exists in the map), v[r] the converted value. */
typedef struct kg_resource_list {
    int64_t v[KG_NUM_RES];
    uint32_t present;
    uint32_t _pad;
} kg_resource_list;

/* ------------------------------------------------------------------ */
/* enums                                                                 */
/* ------------------------------------------------------------------ */
enum kg_priority_class { /* apis/extension/priority.go:28-34 */
    KG_PRIO_NONE = 0,
    KG_PRIO_PROD = 1,
    KG_PRIO_MID = 2,
    KG_PRIO_BATCH = 3,
    KG_PRIO_FREE = 4
};
enum kg_qos_class { /* apis/extension/qos.go */
    KG_QOS_NONE = 0,
    KG_QOS_LSE = 1,
    KG_QOS_LSR = 2,
    KG_QOS_LS = 3,
    KG_QOS_BE = 4,
    KG_QOS_SYSTEM = 5
};
enum kg_kube_qos { /* corev1.PodQOSClass */
    KG_KUBE_QOS_UNSET = 0,
    KG_KUBE_QOS_GUARANTEED = 1,
    KG_KUBE_QOS_BURSTABLE = 2,
    KG_KUBE_QOS_BESTEFFORT = 3
};
enum kg_aggregation_type { /* apis/extension AggregationType */
    KG_AGG_UNSET = 0, /* "" */
    KG_AGG_AVG = 1,
    KG_AGG_P50 = 2,
    KG_AGG_P90 = 3,
    KG_AGG_P95 = 4,
    KG_AGG_P99 = 5
};
#define KG_NUM_AGG_TYPES 6

enum kg_scoring_strategy {
    KG_STRATEGY_LEAST_ALLOCATED = 0,
    KG_STRATEGY_MOST_ALLOCATED = 1
};

#define KG_PLUGIN_FIT 0x1u       /* NodeResourcesFit       */
#define KG_PLUGIN_LOADAWARE 0x2u /* LoadAwareScheduling    */
#define KG_PLUGIN_NUMA 0x4u      /* NodeNUMAResource (zone fit + score, cpuset binding) */
#define KG_PLUGIN_RESERVATION 0x8u  /* Reservation (restore, Filter, Score + NormalizeScore, Reserve) */
#define KG_PLUGIN_ELASTICQUOTA 0x10u /* ElasticQuota (PreFilter quota gate, Reserve used accounting) */

/* NUMA topology policies (apis/extension/numa_aware.go; node label node.koordinator.sh/numa-topology-policy
 * or the NodeResourceTopology kubelet policy, pkg/scheduler/plugins/nodenumaresource/util.go:52-58) */
/* CPU bind policies of NodeNUMAResource (apis/extension/numa_aware.go:86-118) */
enum kg_cpu_bind_policy {          /* ResourceSpec Required/PreferredCPUBindPolicy, args.DefaultCPUBindPolicy */
    KG_CPU_BIND_UNSET = 0,         /* "" */
    KG_CPU_BIND_DEFAULT = 1,       /* "Default" (the plugin's DefaultCPUBindPolicy) */
    KG_CPU_BIND_FULL_PCPUS = 2,
    KG_CPU_BIND_SPREAD_BY_PCPUS = 3,
    KG_CPU_BIND_CONSTRAINED_BURST = 4,
    KG_CPU_BIND_OTHER = 5,         /* any other annotation value (PreFilter binds nothing for it) */
};
enum kg_cpu_exclusive_policy {     /* ResourceSpec.PreferredCPUExclusivePolicy / CPUInfo.ExclusivePolicy */
    KG_CPU_EXCL_UNSET = 0, KG_CPU_EXCL_NONE = 1, KG_CPU_EXCL_PCPU_LEVEL = 2, KG_CPU_EXCL_NUMA_NODE_LEVEL = 3,
};
enum kg_node_cpu_bind_policy {     /* GetNodeCPUBindPolicy: label node.koordinator.sh/cpu-bind-policy, or the
                                      kubelet static policy with full-pcpus-only (numa_aware.go:314-325) */
    KG_NODE_CPU_BIND_NONE = 0, KG_NODE_CPU_BIND_FULL_PCPUS_ONLY = 1, KG_NODE_CPU_BIND_SPREAD_BY_PCPUS = 2,
};

enum kg_numa_allocate_strategy {   /* label node.koordinator.sh/numa-allocate-strategy (numa_aware.go:52-53, util.go:35-41) */
    KG_NUMA_ALLOC_DEFAULT = 0,     /* label absent: the plugin default (NUMAMostAllocated iff NUMAScoringStrategy.Type is
                                      MostAllocated, util.go:27-33) */
    KG_NUMA_ALLOC_MOST = 1, KG_NUMA_ALLOC_LEAST = 2, KG_NUMA_ALLOC_DISTRIBUTE_EVENLY = 3
};

enum kg_numa_policy {
    KG_NUMA_NONE = 0,
    KG_NUMA_BEST_EFFORT = 1,
    KG_NUMA_RESTRICTED = 2,
    KG_NUMA_SINGLE_NUMA_NODE = 3
};
#define KG_MAX_ZONES 8
#define KG_MAX_NODE_CPUS 1024     /* logical CPUs of one node in kg_cluster_view.cpus */

/* ------------------------------------------------------------------ */
/* engine configuration = plugin args (pkg/scheduler/apis/config/types.go)  */
/* ------------------------------------------------------------------ */
typedef struct kg_config {
    int32_t abi_version;       /* must be KG_ABI_VERSION */
    uint32_t enabled_plugins;  /* KG_PLUGIN_* : enabled at Filter AND Score */
    int32_t weight_fit;        /* profile score weight of NodeResourcesFit    */
    int32_t weight_loadaware;  /* profile score weight of LoadAwareScheduling */

    /* NodeResourcesFitArgs.ScoringStrategy (upstream v1.24.15) */
    int32_t fit_strategy;                  /* kg_scoring_strategy */
    int32_t _pad0;
    int64_t fit_resource_weight[KG_NUM_RES]; /* 0 ⇔ resource not listed */

    /* LoadAwareSchedulingArgs (types.go:30-76) */
    int32_t la_filter_expired_node_metrics;   /* *FilterExpiredNodeMetrics (nil ⇒ 0) */
    int32_t la_has_expiration;                /* NodeMetricExpirationSeconds != nil  */
    int64_t la_expiration_seconds;
    int64_t la_resource_weight[KG_NUM_RES];   /* ResourceWeights (0 ⇔ absent).  Weights on resources other than
                                                 cpu / memory take the exact int64 pair path on every node
                                                 (correct, not the fp64 fast kernels) */
    int64_t la_scaling_factor[KG_NUM_RES];    /* EstimatedScalingFactors (missing key ⇒ 0) */
    kg_resource_list la_usage_thresholds;     /* UsageThresholds */
    kg_resource_list la_prod_usage_thresholds;/* ProdUsageThresholds */
    int32_t la_score_according_prod_usage;    /* ScoreAccordingProdUsage */
    int32_t la_has_aggregated;                /* Aggregated != nil */
    kg_resource_list la_agg_usage_thresholds; /* Aggregated.UsageThresholds */
    int32_t la_agg_usage_type;                /* Aggregated.UsageAggregationType */
    int32_t la_agg_score_type;                /* Aggregated.ScoreAggregationType */
    int64_t la_agg_usage_duration_ns;         /* Aggregated.UsageAggregatedDuration (0 ⇒ max) */
    int64_t la_agg_score_duration_ns;         /* Aggregated.ScoreAggregatedDuration (0 ⇒ max) */

    /* NodeNUMAResourceArgs (types.go:103-114); both scorers weigh ScoringStrategy.Resources
     * (nodenumaresource/scoring.go:38,46) */
    int32_t weight_numa;                      /* profile score weight of NodeNUMAResource */
    int32_t numa_strategy;                    /* ScoringStrategy.Type (node / allocated-zone score) */
    int32_t numa_hint_strategy;               /* NUMAScoringStrategy.Type (per-mask hint score) */
    int32_t numa_default_cpu_bind_policy;     /* DefaultCPUBindPolicy (kg_cpu_bind_policy; v1beta2 default FullPCPUs) */
    int64_t numa_resource_weight[KG_NUM_RES]; /* ScoringStrategy.Resources (0 ⇔ absent) */

    /* engine knobs */
    int32_t device;            /* HIP device ordinal */
    int32_t place_chunk;       /* pods per refresh in kg_place (0 ⇒ default 16; at most KG_PLACE_CHUNK_MAX) */

    /* Reservation (profile weight, config/manager/scheduler-config.yaml:82-91 ships 5000) */
    int32_t weight_reservation;
    /* ElasticQuotaArgs.EnableCheckParentQuota: PreFilter also checks every ancestor group below the root
     * (plugin.go:250-252, plugin_helper.go:281-297 checkQuotaRecursive) */
    int32_t eq_check_parent_quota;
    /* names of the scalar slots KG_RES_EXT0 + i ("" ⇔ unused): the resource-name keys the ingest maps to them,
     * and their place in the sorted-name order the topology merge walks (policy.go:108: Go map order, fixed to
     * sorted names here).  Distinct, not one of the fixed names above. */
    char ext_resource_names[KG_NUM_EXT_RES][KG_RES_NAME_MAX];
} kg_config;

/* ------------------------------------------------------------------ */
/* object-level specs (what the Go plugin reads from its informers)        */
/* ------------------------------------------------------------------ */
typedef struct kg_container {
    kg_resource_list requests;
    kg_resource_list limits;
} kg_container;

typedef struct kg_pod_spec {
    int32_t first_container, n_containers;      /* into kg_cluster_view.containers */
    int32_t first_init_container, n_init_containers;
    kg_resource_list overhead;                  /* present == 0 ⇔ Spec.Overhead == nil */
    int32_t has_priority;                       /* Spec.Priority != nil */
    int32_t priority;
    int32_t label_priority_class;               /* -1 label absent, else kg_priority_class of the label value */
    int32_t label_qos;                          /* -1 label absent, else kg_qos_class of the label value */
    int32_t status_qos;                         /* kg_kube_qos of Status.QOSClass (UNSET ⇒ computed) */
    int32_t is_daemonset;                       /* an OwnerReference of Kind DaemonSet */
    int32_t is_terminated;                      /* util.IsPodTerminated */
    int32_t cpu_bind_required;                  /* annotation scheduling.koordinator.sh/resource-spec
                                                   RequiredCPUBindPolicy (kg_cpu_bind_policy) */
    int64_t name_id;                            /* identity of namespace/name */
    /* Reservation: the pod's owner class (reservation.Match(pod) ⇔ bit owner_class of the reservation's
     * owner_classes; −1 ⇔ matches none) and its required reservation affinity class (−1 ⇔ no
     * scheduling.koordinator.sh/reservation-affinity; else the reservation must have bit affinity_class
     * in affinity_classes: reservationAffinity.Match(fakeNode), transformer.go:348-372) */
    int32_t rsv_owner_class;
    int32_t rsv_affinity_class;
    /* ElasticQuota: index into kg_cluster_view.quotas (−1 ⇔ no quota: PreFilter skips) */
    int32_t quota;
    int32_t non_preemptible;                    /* extension.IsPodNonPreemptible */
    int32_t cpu_bind_preferred;                 /* ResourceSpec.PreferredCPUBindPolicy (kg_cpu_bind_policy) */
    int32_t cpu_exclusive;                      /* ResourceSpec.PreferredCPUExclusivePolicy (kg_cpu_exclusive_policy) */
} kg_pod_spec;

typedef struct kg_aggregated_usage { /* slov1alpha1.AggregatedUsage */
    int64_t duration_ns;
    kg_resource_list usage[KG_NUM_AGG_TYPES];   /* map[AggregationType]ResourceMap */
} kg_aggregated_usage;

typedef struct kg_pod_metric { /* slov1alpha1.PodMetricInfo */
    int64_t name_id;      /* namespace/name */
    int32_t lister_pod;   /* index of the pod in kg_cluster_view.pods, -1 ⇔ podLister NotFound */
    int32_t _pad;
    kg_resource_list usage;
} kg_pod_metric;

typedef struct kg_assigned_pod { /* podAssignCache item */
    int32_t pod;          /* index into kg_cluster_view.pods */
    int32_t _pad;
    int64_t timestamp_ns;
} kg_assigned_pod;

typedef struct kg_node_spec {
    /* framework.NodeInfo */
    kg_resource_list allocatable;   /* Allocatable (scalar keys = ScalarResources keys) */
    kg_resource_list requested;     /* Requested */
    int64_t nonzero_requested[2];   /* NonZeroRequested cpu, memory */
    int32_t allowed_pods;           /* Allocatable.AllowedPodNumber */
    int32_t pod_count;              /* len(NodeInfo.Pods) */
    /* annotation node.koordinator.sh/raw-allocatable: 0 absent, 1 present, -1 unparsable */
    int32_t raw_allocatable_state;
    /* annotation scheduling.koordinator.sh/usage-thresholds: 0 absent, 1 present, -1 unparsable */
    int32_t custom_thresholds_state;
    kg_resource_list raw_allocatable;
    kg_resource_list custom_usage_thresholds;
    kg_resource_list custom_prod_usage_thresholds;
    int32_t custom_has_aggregated;          /* AggregatedUsage != nil */
    int32_t custom_agg_usage_type;
    kg_resource_list custom_agg_usage_thresholds;
    int64_t custom_agg_duration_ns;         /* 0 ⇔ nil/zero */
    /* NodeMetric (nodeMetricLister.Get(node.Name)) */
    int32_t has_node_metric;                /* 0 ⇔ NotFound */
    int32_t has_update_time;                /* Status.UpdateTime != nil */
    int64_t update_time_ns;
    int32_t has_report_interval;            /* Spec.CollectPolicy.ReportIntervalSeconds != nil */
    int32_t has_node_metric_info;           /* Status.NodeMetric != nil */
    int64_t report_interval_seconds;
    kg_resource_list node_usage;            /* Status.NodeMetric.NodeUsage */
    int32_t first_aggregated, n_aggregated; /* Status.NodeMetric.AggregatedNodeUsages */
    int32_t first_pod_metric, n_pod_metric; /* Status.PodsMetric */
    int32_t first_assigned, n_assigned;     /* podAssignCache.podInfoItems[node] */
    int32_t numa;                           /* index into kg_cluster_view.numa, −1 ⇔ no topology options */
    int32_t _pad_numa;
} kg_node_spec;

/* NodeNUMAResource view of one node: TopologyOptions (nodenumaresource/topology_options.go:90-153)
 * and the plugin's NodeAllocation (node_allocation.go). */
typedef struct kg_numa_spec {
    int32_t policy;                                  /* kg_numa_policy (label, else NRT policy) */
    int32_t n_zones;                                 /* len(NUMANodeResources) */
    int32_t zone_id[KG_MAX_ZONES];                   /* NUMANodeResource.Node: the zone's affinity bit (< 64) */
    kg_resource_list zone_total[KG_MAX_ZONES];       /* NUMANodeResources[i].Resources (before amplification) */
    kg_resource_list zone_allocated[KG_MAX_ZONES];   /* allocatedResources[zone] (present == 0 ⇔ none) */
    double cpu_amplification_ratio;                  /* annotation resource-amplification-ratio cpu (≤ 1 ⇔ none) */
    int32_t cpu_topology_valid;                      /* TopologyOptions.CPUTopology: 1 valid (IsValid()), 0 reported but
                                                        invalid, −1 nil (no NodeResourceTopology).  Reserve records
                                                        allocations only when valid; with a cpu amplification ratio
                                                        > 1, 0 makes filterAmplifiedCPUs reject cpu requests
                                                        (plugin.go:359-362, resource_manager.go:390-397) */
    int32_t cpuset_cpus;                             /* |NodeAllocation.allocatedCPUs|: CPUs held by cpuset pods
                                                        (GetAvailableCPUs' allocated, no preferred CPUs) */
    int32_t zone_cpuset_cpus[KG_MAX_ZONES];          /* allocatedCPUs.CPUsInNUMANodes(zone_id[z]) (node_allocation.go:165) */
    /* cpuset binding (the CPU accumulator's inputs): the node's CPU bind policy, TopologyOptions.MaxRefCount,
       and its logical CPUs (CPUTopology.CPUDetails + NodeAllocation.allocatedCPUs + ReservedCPUs) as
       kg_cluster_view.cpus[first_cpu, first_cpu + n_cpus), cpu id = position; n_cpus == 0 ⇔ no detail
       (the count fields above then stand alone) */
    int32_t node_cpu_bind_policy;                    /* kg_node_cpu_bind_policy */
    int32_t max_ref_count;                           /* ≥ 1 */
    int32_t first_cpu, n_cpus;
    int32_t numa_allocate_strategy;                  /* kg_numa_allocate_strategy: which CPUs a Reserve takes */
    int32_t _pad_s;
} kg_numa_spec;

/* One logical CPU of a node (CPUInfo of cpu_topology.go + the node allocation's view of it). */
typedef struct kg_cpu_info {
    int32_t socket, node, core;   /* SocketID, NodeID (NUMA node = zone id), CoreID as reported */
    int32_t refcount;             /* NodeAllocation.allocatedCPUs[cpu].RefCount (0 ⇔ not allocated) */
    int32_t exclusive;            /* its ExclusivePolicy (kg_cpu_exclusive_policy) while allocated */
    int32_t reserved;             /* in TopologyOptions.ReservedCPUs (kubelet / node reservation / system QoS) */
} kg_cpu_info;

/* One reservation as the reservation cache holds it (frameworkext.ReservationInfo). */
enum kg_rsv_policy { /* schedulingv1alpha1.ReservationAllocatePolicy */
    KG_RSV_POLICY_DEFAULT = 0,   /* "" */
    KG_RSV_POLICY_ALIGNED = 1,
    KG_RSV_POLICY_RESTRICTED = 2
};
#define KG_RSV_AVAILABLE 0x1u      /* IsAvailable() && ParseError == nil */
#define KG_RSV_UNSCHEDULABLE 0x2u  /* Spec.Unschedulable || terminating */
#define KG_RSV_ALLOCATE_ONCE 0x4u  /* IsAllocateOnce() */
typedef struct kg_reservation {
    int32_t node;                  /* node index (reservationsOnNode key) */
    uint32_t flags;                /* KG_RSV_* */
    int32_t policy;                /* kg_rsv_policy */
    int32_t n_assigned;            /* len(AssignedPods) */
    uint32_t owner_classes;        /* bit c ⇔ Match(pod) for pods of owner class c */
    uint32_t affinity_classes;     /* bit a ⇔ a reservation-affinity class a selects this reservation */
    /* label scheduling.koordinator.sh/reservation-order as strconv.ParseInt(s, 10, 64) reads it (scoring.go:166-178);
     * 0 ⇔ absent / unparsable.  Domain: every int64.  Negative orders are admitted and precede the positive ones
     * (the smallest non-zero order wins).  0 and INT64_MAX never win: "order != 0 && selectOrder > order" starts
     * from selectOrder = MaxInt64, so a label of 9223372036854775807 reads like no label — INT64_MAX is also the
     * engine's "no order" value, with the same meaning. */
    int64_t order;
    kg_resource_list allocatable;  /* Allocatable; present = ResourceNames */
    kg_resource_list allocated;    /* Allocated */
} kg_reservation;

/* One ElasticQuota group (core.QuotaInfo) as its PreFilter reads it. */
typedef struct kg_quota {
    kg_resource_list used_limit;           /* getQuotaInfoUsedLimit: runtime (EnableRuntimeQuota) or max */
    kg_resource_list used;                 /* Used */
    kg_resource_list min;                  /* CalculateInfo.Min (non-preemptible gate) */
    kg_resource_list non_preemptible_used; /* NonPreemptibleUsed */
    /* ParentName as an index into the same list; -1 ⇔ the parent is the root quota (or is not tracked).
     * Reserve adds the pod's requests to the group and every ancestor (group_quota_manager.go:227-238,
     * :334-354); kg_quota_set rejects indices out of range and chains deeper than KG_QUOTA_MAX_DEPTH. */
    int32_t parent;
    int32_t _pad;
} kg_quota;

typedef struct kg_cluster_view {
    const kg_pod_spec *pods;                 int32_t n_pods;       int32_t _p0;
    const kg_container *containers;          int32_t n_containers; int32_t _p1;
    const kg_node_spec *nodes;               int32_t n_nodes;      int32_t _p2;
    const kg_aggregated_usage *aggregated;   int32_t n_aggregated; int32_t _p3;
    const kg_pod_metric *pod_metrics;        int32_t n_pod_metrics; int32_t _p4;
    const kg_assigned_pod *assigned;         int32_t n_assigned;   int32_t _p5;
    const kg_numa_spec *numa;                int32_t n_numa;       int32_t _p6;
    const kg_reservation *reservations;      int32_t n_reservations; int32_t _p7;
    const kg_quota *quotas;                  int32_t n_quotas;     int32_t _p8;
    const kg_cpu_info *cpus;                 int32_t n_cpus;       int32_t _p9;
} kg_cluster_view;

/* ------------------------------------------------------------------ */
/* engine rows (pod-only / node-only precompute; what the kernels read)    */
/* ------------------------------------------------------------------ */
#define KG_POD_HAS_REQUEST 0x1u    /* Fit: request not all-zero (fit.go fitsRequest early return) */
#define KG_POD_DAEMONSET 0x2u      /* LoadAware.Filter passes (load_aware.go:129) */
#define KG_POD_PROD 0x4u           /* GetPodPriorityClassWithDefault == koord-prod */
#define KG_POD_LA_PROD_SCORE 0x8u  /* prodPod && ScoreAccordingProdUsage (load_aware.go:291) */
#define KG_POD_NUMA_SKIP 0x10u     /* NodeNUMAResource PreFilter skip: all requests zero (plugin.go:225-231) */
#define KG_POD_NUMA_CPU_BIND 0x20u /* PreFilter requestCPUBind: LSE/LSR prod with a FullPCPUs / SpreadByPCPUs
                                      policy and a cpu request (plugin.go:232-262) */
#define KG_POD_NUMA_BIND_INVALID 0x100u /* PreFilter ErrInvalidRequestedCPUs (cpu request not whole cores):
                                           NodeNUMAResource fails on every node */
#define KG_POD_NON_PREEMPTIBLE 0x40u /* ElasticQuota: extension.IsPodNonPreemptible (min gate) */
#define KG_POD_VALID 0x80000000u

typedef struct kg_pod_row {
    int64_t request[KG_NUM_RES];        /* Fit PreFilter request (computePodResourceRequest) */
    int64_t fit_score_request[KG_NUM_RES]; /* Fit score pod request per resource (nonzero cpu/mem) */
    int64_t nonzero_request[2];         /* schedutil.GetNonzeroRequests sum (AssumePod NonZeroRequested delta) */
    int64_t la_estimate[2];             /* EstimatePod(pod)[cpu], [memory] */
    uint32_t request_present;           /* ScalarResources key set of the Fit request */
    uint32_t flags;                     /* KG_POD_* */
    int64_t numa_request[KG_NUM_RES];   /* PodRequestsAndLimits requests (NodeNUMAResource PreFilter,
                                           Reservation podRequests, ElasticQuota podRequest) */
    uint32_t numa_request_present;      /* key set of those requests */
    uint32_t cpu_bind;                  /* PreFilter state: required policy | preferred (effective) policy << 4 |
                                           exclusive policy << 8 (kg_cpu_bind_policy / kg_cpu_exclusive_policy) */
    int32_t rsv_owner_class;            /* kg_pod_spec.rsv_owner_class */
    int32_t rsv_affinity_class;         /* kg_pod_spec.rsv_affinity_class */
    int32_t quota;                      /* kg_pod_spec.quota */
    int32_t elig_class;                 /* node eligibility class (kg_elig_set): 0 unrestricted; k ≥ 1: the pod may
                                           only run on nodes of class k − 1.  kg_build_pod_rows writes 0 */
    int64_t la_estimate_x[KG_NUM_RES - 2]; /* EstimatePod(pod)[r] for r = 2..11 (0 unless resourceWeights name r) */
} kg_pod_row;

#define KG_NODE_VALID 0x1u
#define KG_NODE_HAS_METRIC 0x2u          /* nodeMetricLister found the NodeMetric */
#define KG_NODE_HAS_UPDATE_TIME 0x4u     /* Status.UpdateTime != nil */
#define KG_NODE_LA_PASS_NONPROD 0x8u     /* threshold check result for non-prod pods */
#define KG_NODE_LA_PASS_PROD 0x10u       /* threshold check result for prod pods */
#define KG_NODE_LA_AGG_MISSING 0x20u     /* score aggregation requested but not reported (info) */
#define KG_NODE_NUMA_OPTIONS 0x40u       /* the node has NodeNUMAResource topology options */
#define KG_NODE_NUMA_TOPO_VALID 0x80u    /* CPUTopology valid: Reserve records zone allocations */
#define KG_NODE_NUMA_TOPO_INVALID 0x100u /* CPUTopology reported but invalid (GetAvailableCPUs fails) */

typedef struct kg_node_row {
    int64_t alloc[KG_NUM_RES];          /* NodeInfo.Allocatable */
    int64_t requested[KG_NUM_RES];      /* NodeInfo.Requested */
    int64_t nonzero_requested[2];       /* NodeInfo.NonZeroRequested */
    int64_t la_alloc[2];                /* EstimateNode(node)[cpu], [memory] */
    int64_t la_used[2][2];              /* [nonProd, prod][cpu, memory]: assigned-pod estimates + usage term */
    int64_t metric_update_ns;           /* NodeMetric Status.UpdateTime */
    int32_t pod_count;
    int32_t allowed_pods;
    uint32_t alloc_present;             /* Allocatable.ScalarResources key set */
    uint32_t flags;                     /* KG_NODE_* */
    /* NodeNUMAResource: zones of cpu (milli, amplified) and memory; zone z = affinity bit zone_id[z] */
    int32_t numa_policy;                /* kg_numa_policy */
    int32_t n_zones;                    /* 0 ⇔ no NUMA resources */
    int32_t zone_id[KG_MAX_ZONES];
    int64_t zone_total[KG_MAX_ZONES][2];
    int64_t zone_allocated[KG_MAX_ZONES][2];
    uint32_t zone_keys;                 /* bit 2z+r: zone z's total has resource r (cpu 0, memory 1) */
    uint32_t zone_alloc_keys;           /* bit 2z+r: zone z's allocation has resource r */
    double cpu_amplification_ratio;     /* ≤ 1 ⇔ none */
    /* cpuset pods on the node (the amplified-CPU terms of filterAmplifiedCPUs / scoreWithAmplifiedCPUs /
       getAvailableNUMANodeResources); zero unless the CPU topology is valid */
    int64_t cpuset_milli;               /* cpuset_cpus · 1000 */
    int64_t cpuset_amp_milli;           /* Amplify(cpuset_milli, ratio) */
    int64_t zone_cpuset_amp[KG_MAX_ZONES]; /* Amplify(c, ratio) − c, c = zone z's cpuset CPUs · 1000: added to the
                                              zone's allocated cpu while the zone has an allocation entry */
    /* cpuset binding on a node without a NUMA topology policy (the Filter's Allocate reduces to counts:
       takeCPUs always succeeds on a large enough available set, and the required-policy filter leaves
       whole free cores / one CPU per core with a free CPU) */
    int32_t node_cpu_bind;              /* kg_node_cpu_bind_policy */
    int32_t cpus_per_core;              /* CPUTopology.CPUsPerCore() (0 ⇔ no CPU detail) */
    int32_t cpuset_full_free_cpus;      /* CPUs of the cores whose every CPU is available (getAvailableCPUs) */
    int32_t cpuset_free_cores;          /* cores with at least one available CPU */
    /* LoadAwareScheduling resourceWeights beyond cpu / memory (resources 2..11; zero unless weighted):
       EstimateNode(node)[r] and the [nonProd, prod] node terms of r */
    int64_t la_alloc_x[KG_NUM_RES - 2];
    int64_t la_used_x[2][KG_NUM_RES - 2];
    /* cpusets on a node with a NUMA topology policy (trimNUMANodeResources, allocateCPUSet): the node's
       available CPUs, and per zone its available CPUs, the CPUs of its wholly available cores and its
       cores with an available CPU */
    int32_t cpuset_avail_cpus;
    int32_t _pad_cpu;
    int16_t zone_cpus_avail[KG_MAX_ZONES];
    int16_t zone_cpus_full[KG_MAX_ZONES];
    int16_t zone_cores_free[KG_MAX_ZONES];
    int64_t _pad_row;
} kg_node_row;

/* ------------------------------------------------------------------ */
/* engine                                                                 */
/* ------------------------------------------------------------------ */
typedef struct kg_engine kg_engine;

/* Output of kg_eval (matrix mode).  Any pointer may be NULL (not produced).
 * Columns cover the evaluated node range [B, E) (the shard; the whole snapshot by default),
 * W = ceil((E - B) / 64), column c ⇔ node B + c:
 *   mask     [P][W] uint64: bit (c % 64) of word c/64 ⇔ pod p feasible on node B + c
 *            (AND of every enabled Filter plugin and, for a pod with an elig_class, of its class:
 *            kg_elig_set)
 *   scores   [P][64·W][2] uint8: {NodeResourcesFit score, LoadAwareScheduling score} ∈ [0,100]
 *            (0 where a plugin is disabled; row stride 64·W pairs).  Like the reference, where Score
 *            runs only on the nodes that passed Filter, a score is meaningful only where the pair's
 *            mask bit is set: the planes of a pod failing a node-independent gate (ElasticQuota
 *            PreFilter, a required reservation) keep the per-pair plugin scores of the plain nodes.
 *   numa_scores [P][64·W] uint8: NodeNUMAResource score (when KG_PLUGIN_NUMA is enabled)
 *   top1     [P] uint64: (total+1) << 32 | (0xFFFFFFFF − node) of the best feasible node,
 *            total = Σ weight·score, ties → lowest node index; 0 ⇔ no feasible node
 * Pad columns [E − B, 64·W) of a row: the mask's pad bits (the high bits of its last word) are 0; the
 * pad columns of scores, numa_scores and rsv_scores are unspecified (the kernels store whole vectors).
 * Nothing outside the planes' [P][…] extents is written; a plane whose pointer is NULL is not touched.
 * An empty range (B = E) writes top1 only.
 * When out_on_device != 0 the pointers are device pointers on the engine's device
 * (results stay resident; no copy back).  Device outputs need no pre-zeroing: every in-range cell,
 * every mask pad bit and every top1 key is written whatever the buffer held.  Each device pointer
 * must be 16-byte aligned (the kernels store 16-byte vectors; rows of an odd W leave the mask's
 * vector stores 8-byte aligned inside the plane, which the kernels allow for).
 * (tests/test_matrix_guard_gpu.py holds all of this on guarded buffers.) */
typedef struct kg_eval_out {
    uint64_t *mask;
    uint8_t *scores;
    uint64_t *top1;
    int32_t out_on_device;
    int32_t _pad;
    uint8_t *numa_scores;    /* [P][64·W] NodeNUMAResource score (KG_PLUGIN_NUMA only; may be NULL) */
    uint8_t *rsv_scores;     /* [P][64·W] Reservation score after NormalizeScore (KG_PLUGIN_RESERVATION; may be NULL) */
} kg_eval_out;

int32_t kg_abi_version(void);
/* sizeof() of every ABI struct, in the order of kg_struct_id, for binding checks */
enum kg_struct_id {
    KG_SID_RESOURCE_LIST = 0, KG_SID_CONFIG, KG_SID_CONTAINER, KG_SID_POD_SPEC,
    KG_SID_AGGREGATED_USAGE, KG_SID_POD_METRIC, KG_SID_ASSIGNED_POD, KG_SID_NODE_SPEC,
    KG_SID_CLUSTER_VIEW, KG_SID_POD_ROW, KG_SID_NODE_ROW, KG_SID_EVAL_OUT, KG_SID_NUMA_SPEC,
    KG_SID_RESERVATION, KG_SID_QUOTA, KG_SID_RSV_RESTORED, KG_SID_CPU_INFO, KG_SID_COUNTERS, KG_SID_CYCLE_OUT,
    KG_SID_COUNT
};
int64_t kg_struct_size(int32_t sid);

/* Fill a config with the v1beta2 defaults (pkg/scheduler/apis/config/v1beta2/defaults.go:32-137)
 * and NodeResourcesFit LeastAllocated cpu:1 memory:1, both plugins enabled with weight 1. */
void kg_config_default(kg_config *cfg);
/* Shipped profile overrides (config/manager/scheduler-config.yaml:17-45). */
void kg_config_shipped_profile(kg_config *cfg);
kg_status kg_config_validate(const kg_config *cfg, char *err, int32_t err_len);

/* Host-side row builders (pure CPU, no GPU needed). */
kg_status kg_build_pod_rows(const kg_config *cfg, const kg_cluster_view *view,
                            const int32_t *pod_index, int32_t n, kg_pod_row *out);
kg_status kg_build_node_rows(const kg_config *cfg, const kg_cluster_view *view,
                             const int32_t *node_index, int32_t n, kg_node_row *out);
/* Reserve delta (AssumePod + LoadAware.Reserve + NodeNUMAResource.Reserve zone allocations) applied
 * to a host-side row. */
kg_status kg_row_commit(const kg_config *cfg, kg_node_row *node, const kg_pod_row *pod);
/* Unreserve on a host row: the inverse of kg_row_commit.  Subtracts exactly what the Reserve added - requested[r],
 * nonzero_requested, pod_count - 1, the LoadAware terms la_used / la_used_x (the prod terms for a KG_POD_PROD pod) -
 * with plain int64 subtraction, no clamp.  KG_ERR_STATE (nothing changed) when the row is not KG_NODE_VALID or holds
 * no pod.
 * zone_release ([KG_MAX_ZONES][2] by zone slot, or NULL; KG_PLUGIN_NUMA only) is the pod's recorded zone allocation
 * (PodAllocation.NUMANodeResources; kg_row_numa_alloc at Reserve time).  NodeAllocation.release: for a zone z < n_zones
 * that has an allocation entry (either of its zone_alloc_keys bits) and each r with zone_release[z][r] > 0,
 * zone_allocated[z][r] = max(0, zone_allocated[z][r] - release) and bit 2z + r of zone_alloc_keys is set
 * (quotav1.SubtractWithNonNegativeResult).  Key bits are never cleared (the reference keeps the entry with zero
 * quantities), a zone without an entry is untouched, and the row's cpuset counts are not touched.
 * KG_ERR_INVALID_ARG (nothing changed): a negative amount, a non-zero amount at z >= n_zones, or a non-NULL
 * zone_release with NodeNUMAResource disabled. */
kg_status kg_row_unreserve(const kg_config *cfg, kg_node_row *node, const kg_pod_row *pod,
                           const int64_t *zone_release /* [KG_MAX_ZONES][2] or NULL */);
/* The zone amounts kg_row_commit would record for this pod on this (pre-Reserve) row, by zone slot: all zero where
 * the commit records nothing.  The row is not modified.  A caller that drives Reserve itself keeps the result as the
 * pod's PodAllocation.NUMANodeResources and hands it to kg_row_unreserve / kg_unreserve.  KG_ERR_UNSUPPORTED for a
 * pair that binds a cpuset (kg_row_reserve). */
kg_status kg_row_numa_alloc(const kg_config *cfg, const kg_node_row *node, const kg_pod_row *pod,
                            int64_t *zone_alloc /* [KG_MAX_ZONES][2], by zone slot */);
/* Filter + Score of one (pod, node) pair on host rows, through the same per-pair code the kernels
 * run: the single-node checks of a scheduling cycle (RunFilterPluginsWithNominatedPods for one
 * node, preemption's SelectVictimsOnNode, framework_extender.go:354-372) without a device.
 * Scores are the plugin scores (0..100) of the enabled plugins, 0 otherwise.  kg_row_eval and kg_row_eval_rsv
 * take no engine and ignore kg_pod_row.elig_class (kg_elig_set): the caller applies the class itself. */
kg_status kg_row_eval(const kg_config *cfg, const kg_node_row *node, const kg_pod_row *pod, int64_t now_ns,
                      int32_t *feasible, int32_t *fit_score, int32_t *la_score, int32_t *numa_score);
/* Reserve of a pod that may bind a cpuset, on host rows (NodeNUMAResource.Reserve, plugin.go:375-419):
 * requestCPUBind on the node (util.go:105-122), then resourceManager.Allocate (resource_manager.go:171-195) —
 * allocateResourcesByHint on the Filter's hint with the original requests and allocateCPUSet (:273-360), the
 * CPU accumulator zone by zone — and Update (node_allocation.go:57-100): the taken CPUs' RefCount + 1 and
 * ExclusivePolicy, the zone allocations, AssumePod / LoadAware deltas, and the row's cpuset counts re-derived
 * from `cpus` (the node's logical CPUs as kg_cluster_view.cpus holds them; updated in place).
 * numa_allocate_strategy: kg_numa_allocate_strategy of the node (DEFAULT ⇒ the plugin default from cfg).
 * KG_OK: reserved, taken[n_cpus] marks the cpuset (all zero when the pod binds none);
 * KG_NOT_FOUND: Allocate fails ("not enough cpus available to satisfy request" or a required policy that the
 * take cannot satisfy) — the Reserve fails and nothing is changed (Unreserve + ForgetPod). */
kg_status kg_row_reserve(const kg_config *cfg, kg_node_row *node, const kg_pod_row *pod, kg_cpu_info *cpus,
                         int32_t n_cpus, int32_t max_ref_count, int32_t numa_allocate_strategy, uint8_t *taken);

/* Reservation-aware Filter + Score of one (pod, node) pair on host rows through the kernels' per-pair
 * code (kg_rsv_pair): the node's reservation slots `rsv` (≤ KG_MAX_RSV_PER_NODE, in cache order) are
 * restored for the pod (transformer.go:49-291), Fit / LoadAware / NodeNUMAResource / Reservation.Filter
 * run on the restored NodeInfo, and *rsv_raw / *order / *nominated are the pod's PreScore inputs for this node
 * (scoreReservation of the nominated reservation, its order label, its slot; −1 none).  The
 * preferred-node override and NormalizeScore are per-pod reductions over nodes (not per pair). */
kg_status kg_row_eval_rsv(const kg_config *cfg, const kg_node_row *node, const kg_reservation *rsv, int32_t n_rsv,
                          const kg_pod_row *pod, int64_t now_ns, int32_t *feasible, int32_t *fit_score,
                          int32_t *la_score, int32_t *numa_score, int32_t *rsv_raw, int64_t *order,
                          int32_t *nominated);

/* The Reservation restore of one (pod, node) pair as the plugins see it (BeforePreFilter,
 * transformer.go:49-291): NodeInfo after restoring the unmatched reservations' remainders and removing
 * the matched reserve pods, and the nodeReservationState the Filter / nomination read. */
typedef struct kg_rsv_restored {
    int64_t requested[KG_NUM_RES];      /* NodeInfo.Requested after the restore */
    int64_t pod_requested[KG_NUM_RES];  /* nodeRState.podRequested (after the unmatched part) */
    int64_t r_allocated[KG_NUM_RES];    /* nodeRState.rAllocated (Σ Allocated of the matched) */
    int64_t nonzero[2];                 /* NodeInfo.NonZeroRequested after the restore */
    int32_t pod_count;                  /* len(NodeInfo.Pods) after the restore */
    int32_t n_matched;                  /* matched reservations (their slots: rsv[] order) */
    int32_t has_state;                  /* nodeReservationStates has the node */
    int32_t _pad;
} kg_rsv_restored;
kg_status kg_row_rsv_restore(const kg_config *cfg, const kg_node_row *node, const kg_reservation *rsv, int32_t n_rsv,
                             const kg_pod_row *pod, kg_rsv_restored *out);

/* Engine lifecycle. */
kg_status kg_engine_create(const kg_config *cfg, kg_engine **out);
void kg_engine_destroy(kg_engine *eng);
const char *kg_last_error(const kg_engine *eng);
kg_status kg_set_stream(kg_engine *eng, void *hip_stream); /* NULL ⇒ engine-owned stream */
kg_status kg_sync(kg_engine *eng);

/* Node snapshot (HBM-resident). */
kg_status kg_snapshot_reset(kg_engine *eng, int32_t n_nodes);
/* kg_snapshot_upsert writes rows[k] to node node_index[k], k < n, and derives the node's planes from it.  The
 * entries apply in order: where one call names an index more than once, the last entry for that index wins (row,
 * planes and cpuset-binding facts alike) and the earlier ones leave no trace.  Every entry is validated, superseded
 * ones included; an invalid one fails the call and changes nothing.  n = 0 is a no-op. */
kg_status kg_snapshot_upsert(kg_engine *eng, const int32_t *node_index, const kg_node_row *rows, int32_t n);
kg_status kg_snapshot_remove(kg_engine *eng, int32_t node_index);
kg_status kg_snapshot_download(kg_engine *eng, int32_t first, int32_t n, kg_node_row *out);
/* Snapshot generation (SURVEY §5 error contract; replaces the Go cache's generation check in
 * Cache.UpdateSnapshot, a per-cycle staleness test): the count of successful snapshot mutations —
 * kg_snapshot_reset, kg_snapshot_upsert / _remove, kg_commit, a committing kg_cycle_one, a kg_unreserve that released
 * an entry and each placement resolve (kg_place, kg_place_chunk_resolve).  After a HIP error the device state is stale: this returns KG_ERR_STATE (with
 * the generation reached), every other entry point fails with KG_ERR_STATE, and the caller falls back to
 * the CPU plugins until kg_snapshot_reset + upsert reload the snapshot. */
kg_status kg_snapshot_generation(kg_engine *eng, uint64_t *out);

/* NodeNUMAResource's CPU accumulator on one node's logical CPUs: the cpuset a Reserve takes
 * (takeCPUs, nodenumaresource/cpu_accumulator.go:87-822) from `available` (per cpu id), with the node's
 * allocated CPUs' RefCount / ExclusivePolicy from `cpus`.  bind_policy / exclusive_policy:
 * kg_cpu_bind_policy / kg_cpu_exclusive_policy; numa_strategy: kg_scoring_strategy (NUMAAllocateStrategy).
 * KG_OK ⇔ `need` CPUs marked in result[n_cpus]; KG_NOT_FOUND ⇔ the accumulator fails.  The engine runs the
 * same code at Reserve in kg_place / kg_commit; exposed for host tools and tests. */
kg_status kg_cpuset_take(const kg_cpu_info *cpus, int32_t n_cpus, int32_t max_ref_count, const uint8_t *available,
                         int32_t need, int32_t bind_policy, int32_t exclusive_policy, int32_t numa_strategy,
                         uint8_t *result);
/* The logical CPUs of snapshot nodes (NodeNUMAResource's NodeAllocation.allocatedCPUs + CPUTopology +
 * ReservedCPUs, with MaxRefCount and the node's NUMA allocate strategy): for k < n, snapshot node
 * snap_index[k] takes the CPU detail of view node view_index[k] (either array NULL ⇔ k itself); a listed node
 * without CPU detail loses its table, unlisted nodes keep theirs (the feeders push the nodes an event
 * changed, next to their rows).  kg_snapshot_reset drops every table, kg_snapshot_remove the node's.
 * kg_place / kg_commit take cpusets from these tables at Reserve (the host runs the CPU accumulator for the
 * chosen node between device chunks) and write the node's cpuset counts back to its row.
 * kg_cpus_download reads one node's table (n = its CPU count). */
kg_status kg_cpus_set(kg_engine *eng, const kg_cluster_view *view, const int32_t *view_index, const int32_t *snap_index,
                      int32_t n);
kg_status kg_cpus_download(kg_engine *eng, int32_t node, kg_cpu_info *out, int32_t n);
/* Restrict kg_eval/kg_place evaluation to nodes [begin, end) (node sharding across GPUs);
 * node indices stay global.  begin must be a multiple of 1024 unless the shard is empty. */
kg_status kg_set_shard(kg_engine *eng, int32_t begin, int32_t end);

/* Pod batch (uploaded once; HBM-resident until replaced). */
kg_status kg_pods_set(kg_engine *eng, const kg_pod_row *pods, int32_t n_pods);

/* The slot map kg_pods_set chooses for a batch (host only, no engine): the resources the fp64 slot kernels carry.
 * A pod "needs" a resource when the Fit filter compares it (a native with a non-zero request, a scalar whose key
 * is present) or NodeResourcesFit scores it (weighted, and for a scalar a non-zero score request).  Over the union
 * of the pods' needs:
 *   - within {cpu, memory}: 2 slots; within {cpu, memory, batch-cpu, batch-memory}: those 4 slots;
 *   - at most 8 resources: 8 slots, cpu and memory then the others in ascending resource id (unused slots −1);
 *   - more than 8: cpu, memory and the 6 other resources that the most pods need (ties to the lower resource id),
 *     stored in ascending resource id.  A pod that needs a resource outside the map is a spill pod (spill[i] = 1;
 *     a pod that alone needs more than 8 always is): the engine evaluates it on the generic pair path, which
 *     answers all KG_NUM_RES resources, so its results do not depend on the map.
 * The rule is deterministic.  n_slots ← 2, 4 or 8; slot_res[8] ← resource id per slot; spill (n bytes, may be
 * NULL) ← 0 / 1 per pod, all zero unless the union exceeds 8. */
kg_status kg_batch_slot_map(const kg_config *cfg, const kg_pod_row *pods, int32_t n, int32_t *n_slots,
                            int32_t slot_res[8], uint8_t *spill);
/* Spill pods of the batch uploaded with kg_pods_set (0 for every batch of at most 8 resources). */
int32_t kg_pods_spill_count(const kg_engine *eng);

/* Node eligibility classes: the verdicts of the Filter plugins the engine does not model (NodeAffinity /
 * nodeSelector, TaintToleration, NodeName, NodeUnschedulable, ...), one bit per (class, node).  A pod row with
 * elig_class = k ≥ 1 is feasible only on the nodes whose bit is set in class k − 1; the bit is ANDed into the
 * pair's feasibility on every path where the engine chooses or reports a node (kg_eval's mask and top1, kg_place,
 * kg_place_sharded, the chunk API, kg_cycle_one).  Plugin scores stay the pair's own (meaningful where the mask
 * bit is set).  elig_class = 0 is unrestricted.
 * kg_elig_set replaces the whole table: masks is [n_classes][ceil(n_nodes / 64)] uint64, bit (n % 64) of word
 * n / 64 of a class's row ⇔ node n (global snapshot index, also under kg_set_shard) is eligible; bits past
 * n_nodes are ignored.  n_classes = 0 drops the table.  n_nodes must be the snapshot size (KG_ERR_RANGE);
 * without a snapshot KG_ERR_STATE.  kg_snapshot_reset drops the table; kg_snapshot_upsert / kg_snapshot_remove
 * leave it alone.  Under kg_place_sharded every rank loads the same table.
 * kg_elig_update sets (eligible[i] != 0) or clears the bit of nodes[i] in class cls, i < n: the node-event path.
 * An out-of-range class or node returns KG_ERR_RANGE and changes nothing.
 * A batch (or a kg_cycle_one pod) that names a class at or past the loaded count, or a negative one, makes
 * kg_eval, kg_place, kg_place_sharded, the chunk entry points and kg_cycle_one return KG_ERR_RANGE before anything
 * is launched or changed.  kg_commit(pod, node) does not check eligibility: the node is the caller's decision.
 * kg_pods_restricted_count: pods of the uploaded batch with elig_class != 0 (they take the generic pair path,
 * k_eval_elig, like spill pods; kg_pods_spill_count keeps counting the pods outside the slot map only). */
kg_status kg_elig_set(kg_engine *eng, const uint64_t *masks, int32_t n_classes, int32_t n_nodes);
kg_status kg_elig_update(kg_engine *eng, int32_t cls, const int32_t *nodes, const uint8_t *eligible, int32_t n);
int32_t kg_pods_restricted_count(const kg_engine *eng);

/* Matrix mode: every (pod, node) Filter+Score of the uploaded batch against the snapshot. */
kg_status kg_eval(kg_engine *eng, int64_t now_ns, const kg_eval_out *out);

/* Placement mode: schedule the uploaded batch in queue order exactly like the sequential
 * cycle (Filter all nodes → Score → argmax, lowest index on ties → Reserve), committing
 * each placement to the snapshot.  out_node[p] = node or −1, out_score[p] = total score
 * (−1 when unschedulable, or when its Reserve fails: a cpuset the CPU accumulator cannot take).
 * Pods that may bind a cpuset end their device chunk; their Reserve takes the CPUs on the host
 * (kg_cpus_set tables) before the next chunk is evaluated. */
kg_status kg_place(kg_engine *eng, int64_t now_ns, int32_t *out_node, int64_t *out_score);

/* Native multi-GPU placement: one engine per GPU, each holding the whole (replicated) snapshot and
 * restricted to its node shard (kg_set_shard).  kg_comm_unique_id (one rank) makes the RCCL id every rank passes
 * to kg_comm_init (librccl is loaded on first use; KG_ERR_UNSUPPORTED without it).  kg_place_sharded is kg_place
 * over the shards: per chunk each rank evaluates its tiles, the chunk's per-(pod, tile) partial keys are merged
 * with one ncclAllReduce(max) on the engine stream (beside the resolve in the pipelined form), and every rank runs
 * the same resolve and host Reserve steps (cpusets included) on identical inputs, so the replicas stay identical
 * and the placements equal kg_place's.  Every rank calls it with the same batch; outputs as kg_place. */
#define KG_COMM_ID_BYTES 128
kg_status kg_comm_unique_id(void *out /* KG_COMM_ID_BYTES */);
kg_status kg_comm_init(kg_engine *eng, int32_t rank, int32_t world, const void *unique_id);
/* The loopback communicator: the ranks (processes of one host, on one GPU or several) merge the partial keys
 * through a POSIX shared-memory segment `name` ("/…", the same on every rank; unlinked once every rank has joined)
 * instead of RCCL, running the same chunk loop — the rehearsal of kg_place_sharded where RCCL cannot form a
 * communicator (two ranks on one device).  Needs the snapshot loaded (the slots follow its tile count); a rank that
 * does not arrive within 120 s fails the others' waits with KG_ERR_STATE instead of hanging them. */
kg_status kg_comm_init_loopback(kg_engine *eng, int32_t rank, int32_t world, const char *name);
#define KG_COMM_NONE 0
#define KG_COMM_RCCL 1
#define KG_COMM_LOOPBACK 2
int32_t kg_comm_kind(const kg_engine *eng);
/* Failure contract: the ranks first agree (one status all-reduce) that each set up its loop; if any failed, none
 * enters it — that rank returns its error, the others KG_ERR_STATE, nothing is placed.  A step that fails inside
 * the loop (not a HIP fault) turns the rest of that rank's loop into merges of zero keys flagged as failed, so no
 * peer blocks in a collective; every rank then returns an error and is stale (reload the snapshot).  A HIP fault
 * leaves the device unusable: RCCL peers may then block in their next collective (loopback peers time out). */
kg_status kg_place_sharded(kg_engine *eng, int64_t now_ns, int32_t *out_node, int64_t *out_score);

/* Multi-GPU building blocks of kg_place (see koordinator_amd/dist.py); pods that bind cpusets are refused
 * here (KG_ERR_UNSUPPORTED: the sharded resolve has no host Reserve step):
 * chunk_eval writes per-(pod, 1024-node tile) partial keys of the shard for pods
 * [pod_begin, pod_begin+n) into partial_dev ([n][tiles_total][KG_PARTIAL_SLOTS] uint32, tile index
 * global; the caller zeroes nothing, chunk_eval clears the buffer's n rows itself);
 * chunk_resolve commits those pods sequentially given the partials of ALL tiles. */
int32_t kg_num_tiles(const kg_engine *eng);
kg_status kg_place_chunk_eval(kg_engine *eng, int64_t now_ns, int32_t pod_begin, int32_t n, uint32_t *partial_dev);
kg_status kg_place_chunk_resolve(kg_engine *eng, int64_t now_ns, int32_t pod_begin, int32_t n,
                                 const uint32_t *partial_dev, int32_t *out_node_dev, int64_t *out_score_dev);
/* The pipelined form (dist.place_sharded): chunk i + 1 is evaluated — on the eval stream, beside its partial
 * merge — while chunk i is resolved on the engine stream, so its partials may predate chunk i's commits.
 * kg_place_chunk_resolve_prev takes the nodes chunk i placed (prev_nodes_dev[0..n_prev), device, −1 = none)
 * and re-scores them like nodes this chunk touches (their keys in the lists are not trusted), exactly as the
 * one-GPU kg_place pipeline does.  The caller orders the streams: eval(i + 1) after resolve(i − 1), resolve(i)
 * after eval(i) and its merge.  Not with reservations (their per-pod entries are written by chunk_eval).
 * kg_set_eval_stream: the stream kg_place_chunk_eval launches on (NULL ⇒ the engine stream); no sync.  A resolve
 * waits (on the device) for the kg_place_chunk_eval that last wrote its partial_dev, not for later evaluations. */
kg_status kg_place_chunk_resolve_prev(kg_engine *eng, int64_t now_ns, int32_t pod_begin, int32_t n,
                                      const uint32_t *partial_dev, int32_t *out_node_dev, int64_t *out_score_dev,
                                      const int32_t *prev_nodes_dev, int32_t n_prev);
kg_status kg_set_eval_stream(kg_engine *eng, void *hip_stream);

/* Kernel forms the engine picks by batch and snapshot size, forced so that parity tests reach each form on
 * small clusters (0, the default: chosen by size).  Every form answers identically.
 *  KG_FORM_PLACE_PIPELINE    kg_place evaluates chunk i + 1 beside chunk i's resolve for every batch (by size:
 *                            NodeNUMAResource batches, whose chunk evaluation is long)
 *  KG_FORM_PLACE_SEQUENTIAL  kg_place never pipelines
 *  KG_FORM_NUMA_QUEUED       NodeNUMAResource matrix launches take the queued work-item form (by size: launches
 *                            with at least one work item per resident wave, and placement chunks)
 *  KG_FORM_NUMA_CHUNK_TILE   NodeNUMAResource placement chunks write one key per tile through the matrix kernel
 *                            (by size: chunks above 16 pods; smaller ones take per-tile top-16 lists)
 *  KG_FORM_NUMA_NO_CACHE     pipelined NodeNUMAResource placement evaluates every chunk pair by pair (by size: a
 *                            batch of repeated pod rows reads the distinct rows' outcomes from a per-node cache,
 *                            refreshed for each chunk's committed nodes)
 *  KG_FORM_NUMA_FUSED        NodeNUMAResource matrix launches evaluate Fit + LoadAware inside k_eval_numa2 (by size:
 *                            a matrix launch with planes runs the Fit + LoadAware pass first and k_eval_numa2
 *                            adds the NodeNUMAResource term to its planes) */
#define KG_FORM_PLACE_PIPELINE 0x1u
#define KG_FORM_PLACE_SEQUENTIAL 0x2u
#define KG_FORM_NUMA_QUEUED 0x4u
#define KG_FORM_NUMA_CHUNK_TILE 0x8u
#define KG_FORM_NUMA_NO_CACHE 0x10u
#define KG_FORM_NUMA_FUSED 0x20u
kg_status kg_set_forms(kg_engine *eng, uint32_t forms);

/* Reservation cache (KG_PLUGIN_RESERVATION): replaces every reservation slot; a node holds at most
 * KG_MAX_RSV_PER_NODE.  Nodes carrying slots are evaluated on the exact per-pair path with the
 * restore of transformer.go:49-291.  Under kg_set_shard every rank still evaluates every reservation
 * node (the slots are replicated): the per-pod preferred-reservation choice and Reservation
 * NormalizeScore's maximum (plugin.go Score / NormalizeScore) are global and identical on each rank,
 * the planes cover the shard's columns only, and top1 includes every reservation node, so a max over
 * the ranks' top1 keys equals the unsharded result.
 * kg_rsv_download returns the slots (allocated / n_assigned after placements) in kg_rsv_set order. */
#define KG_MAX_RSV_PER_NODE 16
kg_status kg_rsv_set(kg_engine *eng, const kg_reservation *rsv, int32_t n);
kg_status kg_rsv_download(kg_engine *eng, kg_reservation *out, int32_t n);
/* ElasticQuota groups (KG_PLUGIN_ELASTICQUOTA); kg_pod_row.quota indexes them. */
kg_status kg_quota_set(kg_engine *eng, const kg_quota *q, int32_t n);
kg_status kg_quota_download(kg_engine *eng, kg_quota *out, int32_t n);

/* Single Reserve on the device snapshot (pod = index in the uploaded batch); a cpuset pod takes its CPUs
 * from the node's kg_cpus_set table.  KG_NOT_FOUND ⇔ its Allocate fails (nothing changed). */
kg_status kg_commit(kg_engine *eng, int32_t pod, int32_t node);

/* Batched Unreserve on the device snapshot: entry i undoes the Reserve of pods[i] on nodes[i] (kg_commit, a committing
 * kg_cycle_one, a kg_place / kg_place_sharded placement).  The pod rows travel with the call (as kg_cycle_one and
 * kg_diagnose); the batch uploaded with kg_pods_set is neither read nor replaced.  Node indices are global and the
 * shard is ignored (as kg_commit).  Entries may repeat a node, a reservation slot or a quota group; the result is the
 * same as applying the entries one by one in call order.
 * Node part: kg_row_unreserve (with zone_release + i * KG_MAX_ZONES * 2 when given) on the node's row, then every
 * plane and flag re-derived as kg_snapshot_upsert would from the new row.  A node is all-or-nothing: when it is not
 * valid (removed), holds fewer pods than the call releases from it, or one of its entries names an invalid slot, none
 * of its entries is applied and each gets released[i] = 0; the other nodes proceed (released[i] = 1).
 * Reservation part (Reservation enabled, slots loaded, rsv_slot[i] >= 0: the kg_rsv_set index the Reserve nominated,
 * kg_row_eval_rsv's *nominated): with m = numa_request_present & allocatable.present, allocated.v[q] =
 * max(0, allocated.v[q] - numa_request[q]) for q in m, allocated.present |= m, n_assigned - 1.  A slot is invalid for
 * an entry when its node is not nodes[i] or its n_assigned is smaller than the number of entries naming it.
 * ElasticQuota part (released entries only): numa_request subtracted from `used` of the pod's group and every
 * ancestor, and from non_preemptible_used for a KG_POD_NON_PREEMPTIBLE pod.
 * Errors (nothing launched, nothing changed): KG_ERR_INVALID_ARG for n < 0, a null pods / nodes / released with n > 0,
 * flags != 0, or zone arguments kg_row_unreserve refuses; KG_ERR_RANGE for n > KG_UNRESERVE_MAX, a node outside the
 * snapshot, a slot at or past the loaded count, or a pod row outside the engine bounds; KG_ERR_STATE without a
 * snapshot, on a stale engine, for a quota index without a kg_quota_set group, or rsv_slot[i] >= 0 with no slots
 * loaded; KG_ERR_UNSUPPORTED under NodeNUMAResource for a pod with KG_POD_NUMA_CPU_BIND or a snapshot holding a node
 * with a CPU bind policy (kg_cycle_one's rule: a cpuset release needs the CPU table; those cycles keep
 * kg_snapshot_upsert + kg_cpus_set).
 * On success: n = 0 is a no-op; the generation goes up by 1 when at least one entry was released; kg_counters.placed
 * is unchanged, h2d_bytes grows by the bytes uploaded; the call returns after the launches completed.
 * Under kg_place_sharded every rank calls it with the same arguments, so the replicas stay identical.
 * Contract: the release is exact for a Reserve whose node row the engine still holds.  After a kg_snapshot_upsert of
 * that node the host row is the truth (it was built without the pod, or the caller rebuilds it so): the caller must
 * not also release. */
#define KG_UNRESERVE_MAX 4096
kg_status kg_unreserve(kg_engine *eng, const kg_pod_row *pods, const int32_t *nodes, int32_t n, uint32_t flags,
                       const int64_t *zone_release /* [n][KG_MAX_ZONES][2] or NULL */,
                       const int32_t *rsv_slot     /* [n], kg_rsv_set index or -1; or NULL */,
                       uint8_t *released           /* [n] out, host */);

/* Gang-aware placement: kg_place over the uploaded batch with Coscheduling's all-or-nothing rejection applied inside
 * the batch.  pod_gang[p] names the gang of pod p (-1: none, a plain pod; pass -1 too for a once-satisfied gang or one
 * the caller does not want enforced); gang_min[g] is max(0, MinRequiredNumber - members already waiting or bound
 * outside this batch) (the caller's reading of isGangValidForPermit, gang.go:480-495); gang_group[g] is the gang
 * group of g as an index in [0, n_gangs) (NULL: every gang is its own group); gang_flags[g] is KG_GANG_STRICT
 * (extension.GangModeStrict) or 0.  PodGroup bookkeeping, timeouts and match policies stay with the caller.
 * For each pod p in queue order, with g = pod_gang[p], G its group and rejected[G] false at the start:
 *  1. g strict and rejected[G]: out_node[p] = out_score[p] = -1; the pod is not evaluated and leaves no trace on rows,
 *     planes or quota state (PreFilter of an invalid schedule cycle, coscheduling/core/core.go:255-269).
 *  2. Otherwise one cycle exactly as kg_place runs it on the snapshot of that moment (eligibility classes, spill
 *     pods, the ElasticQuota gate on the current `used`, the lowest node index on ties, the Reserve).
 *  3. The cycle finds no node (for any reason, the quota gate included) and g is strict: rejected[G] is set and every
 *     earlier pod q < p of a gang of G with out_node[q] >= 0 is unreserved exactly as kg_unreserve(pods[q],
 *     out_node[q]) would (row, every derived plane, ElasticQuota used / non_preemptible_used up the parent chain) and
 *     gets out_node[q] = out_score[q] = -1 (rejectGangGroupById, core.go:276-306, :343-388).  All of this is complete
 *     before pod p + 1's cycle: the reference rejects the waiting pods asynchronously, "before the next pod" is this
 *     engine's deterministic rule.
 *  4. A non-strict member without a node is simply unschedulable (core.go:305).
 *  5. After the last pod, gang g is satisfied iff its pods with out_node >= 0 number at least gang_min[g];
 *     out_verdict[g] is its group's verdict: KG_GANG_REJECTED if rejected[G], else KG_GANG_ALLOWED if every gang of G
 *     is satisfied, else KG_GANG_WAITING (its Reserves stay: the pods wait in Permit).  With
 *     KG_PLACE_GANG_RELEASE_WAITING the WAITING groups, strict or not, are rolled back as in rule 3 (the Permit
 *     timeout); their verdict stays KG_GANG_WAITING.
 *  6. n_gangs = 0, or every pod_gang = -1, gives exactly kg_place.  Results do not depend on kg_config.place_chunk
 *     or kg_set_forms: a gang batch always takes the sequential chunk loop, with chunks cut as kg_gang_plan reports.
 * Errors (nothing launched, nothing changed): KG_ERR_INVALID_ARG for a null pod_gang / out_node / out_score with pods
 * uploaded, a null gang_min / gang_flags / out_verdict with n_gangs > 0, n_gangs < 0, unknown flags or gang_flags
 * bits, a negative gang_min, or gangs of one group that disagree on KG_GANG_STRICT; KG_ERR_RANGE for a pod_gang outside
 * [-1, n_gangs) or a gang_group outside [0, n_gangs); KG_ERR_STATE as kg_place (no snapshot, a stale engine, a shard
 * set, a quota index without a group); KG_ERR_UNSUPPORTED with KG_PLUGIN_NUMA enabled (the release needs the recorded
 * zone allocations and cpusets) or Reservation enabled with slots loaded (it needs the nominated slot).
 * kg_counters.placed grows by the pods with out_node >= 0 at return; the generation moves as in kg_place (once per
 * resolved chunk), so it is unchanged exactly when nothing was launched. */
#define KG_GANG_STRICT 0x1u /* gang_flags */
#define KG_GANG_ALLOWED 0   /* out_verdict */
#define KG_GANG_WAITING 1
#define KG_GANG_REJECTED 2
#define KG_PLACE_GANG_RELEASE_WAITING 0x1u /* flags */
kg_status kg_place_gangs(kg_engine *eng, int64_t now_ns,
                         const int32_t *pod_gang   /* [P] gang index of each pod of the uploaded batch, -1: none */,
                         const int32_t *gang_min   /* [n_gangs] members this batch must still place for Permit */,
                         const int32_t *gang_group /* [n_gangs] gang-group index in [0, n_gangs); NULL: gang g is group g */,
                         const uint8_t *gang_flags /* [n_gangs] KG_GANG_STRICT or 0 */,
                         int32_t n_gangs, uint32_t flags,
                         int32_t *out_node, int64_t *out_score /* [P], as kg_place */,
                         uint8_t *out_verdict /* [n_gangs] */);

/* Host only, no engine: the argument checks above that need no engine (pod_gang, gang_group, gang_flags, n_gangs;
 * n_pods < 0 or a null cut with n_pods > 0: KG_ERR_INVALID_ARG) and the chunk cuts kg_place_gangs will use for
 * place_chunk = chunk (<= 0: the default 16; clamped to KG_PLACE_CHUNK_MAX): cut[p] = 1 when a placement chunk ends
 * after pod p.  A chunk is at most `chunk` consecutive pods that are all members of one strict gang group or hold
 * no strict-gang pod.  On an error cut is untouched. */
kg_status kg_gang_plan(const int32_t *pod_gang, int32_t n_pods, const int32_t *gang_group, const uint8_t *gang_flags,
                       int32_t n_gangs, int32_t chunk, uint8_t *cut /* [n_pods] */);

/* One scheduling cycle of one pod (upstream scheduleOne: Filter and Score over every node of the shard,
 * selectHost, Reserve) as ONE kernel launch and ONE stream synchronisation: the per-pod loop of the Go plugins
 * without kg_pods_set + kg_eval + kg_commit.  The pod row travels with the launch; the batch uploaded with
 * kg_pods_set is neither read nor replaced.
 * Selection is exactly kg_pods_set(pod, 1) + kg_eval(top1): the shard of kg_set_shard, ties to the lowest node
 * index, the exact int64 pair path for nodes outside the fp64 bounds, for the later named slots and for LoadAware
 * weights beyond cpu / memory.  With KG_CYCLE_COMMIT the chosen node is reserved in the same launch exactly as
 * kg_commit(pod, node) would (snapshot generation + 1, kg_counters.placed + 1); without a feasible node nothing
 * changes.
 * planes (may be NULL): mask / scores / numa_scores receive the pod's planes in kg_eval's P = 1 layout (host or
 * device pointers by out_on_device), top1 the key; rsv_scores must be NULL.  They describe the snapshot before
 * the commit.
 * KG_ERR_UNSUPPORTED (nothing launched, nothing changed) — keep the three-call path — when Reservation is enabled
 * with reservation slots loaded, when ElasticQuota is enabled, and under NodeNUMAResource for a pod that binds a
 * cpuset (KG_POD_NUMA_CPU_BIND) or a snapshot holding a node with a CPU bind policy. */
#define KG_CYCLE_COMMIT 0x1u       /* Reserve the chosen node in the same launch */
typedef struct kg_cycle_out {
    uint64_t key;        /* as kg_eval_out.top1: (total+1) << 32 | (0xFFFFFFFF - node); 0 <=> no feasible node */
    int32_t  node;       /* chosen node (global index), -1 when none */
    int32_t  committed;  /* 1 <=> the Reserve was applied to the snapshot */
    int64_t  score;      /* total score, -1 when none (kg_place's out_score convention) */
} kg_cycle_out;
kg_status kg_cycle_one(kg_engine *eng, const kg_pod_row *pod, int64_t now_ns, uint32_t flags,
                       const kg_eval_out *planes /* may be NULL */, kg_cycle_out *out);

/* Rejection reasons: why a pod fits nowhere (upstream findNodesThatPassFilters' Diagnosis.NodeToStatusMap, the
 * FailedScheduling event "0/N nodes are available: 312 Insufficient cpu, 97 Too many pods, ...", and the
 * candidate nodes of preemption).  The reason word of a (pod, node) pair is a uint32 of KG_WHY_* bits, zero exactly
 * when the pair is feasible (kg_eval's mask bit):
 *   KG_WHY_ABSENT      the row is not KG_NODE_VALID (a removed node); no other bit is set then
 *   KG_WHY_ELIG        the pod has elig_class = k >= 1 and the node's bit in class k - 1 is clear (kg_elig_set)
 *   KG_WHY_FIT_PODS    NodeResourcesFit: pod_count + 1 > allowed_pods ("Too many pods")
 *   KG_WHY_LOADAWARE   LoadAwareScheduling rejects the node for the pod's prod / non-prod variant (not a daemonset
 *                      pod; NodeMetric expiry is judged at now_ns)
 *   KG_WHY_NUMA        NodeNUMAResource: the pair is infeasible (not for a KG_POD_NUMA_SKIP pod)
 *   KG_WHY_FIT_RES(r)  NodeResourcesFit, a pod with KG_POD_HAS_REQUEST: resource r is compared (r < 3, or bit r of
 *                      request_present) and request[r] > alloc[r] - requested[r] ("Insufficient <r>").  Every
 *                      failing resource is reported, not the first (upstream fitsRequest collects them all), and a
 *                      zero cpu / memory / ephemeral-storage request fails where alloc - requested is negative.
 * Every enabled plugin is evaluated on its own.  With KG_DIAG_FIRST_FAIL the word keeps only the bits of the first
 * failing group in the reference's filter order - ABSENT, ELIG, NodeResourcesFit (all of its bits), LOADAWARE,
 * NUMA: the default plugins, then config/manager/scheduler-config.yaml:65-70 - which is what NodeToStatusMap
 * holds for the node; the NodeNUMAResource pair is then not evaluated where an earlier group failed.
 * The pod-level word (KG_WHY_POD_*) holds the gates that do not depend on the node; the per-node words and
 * counts do not include them (as the score planes):
 *   KG_WHY_POD_QUOTA         ElasticQuota is enabled and the pod fails its PreFilter against the engine's quota
 *                            state (kg_quota_set and the commits since; eq_check_parent_quota included)
 *   KG_WHY_POD_RSV_REQUIRED  the pod requires a reservation and no reservation slots are loaded */
#define KG_WHY_ABSENT 0x1u
#define KG_WHY_ELIG 0x2u
#define KG_WHY_FIT_PODS 0x4u
#define KG_WHY_LOADAWARE 0x8u
#define KG_WHY_NUMA 0x10u
#define KG_WHY_FIT_RES_SHIFT 16
#define KG_WHY_FIT_RES(r) (1u << (KG_WHY_FIT_RES_SHIFT + (r)))   /* r < KG_NUM_RES */
#define KG_WHY_POD_QUOTA 0x1u
#define KG_WHY_POD_RSV_REQUIRED 0x2u
#define KG_DIAG_FIRST_FAIL 0x1u
/* The reason word of one pair on host rows (no engine), as kg_row_eval: the single-node checks (preemption's
 * SelectVictimsOnNode) without a device.  flags: 0 or KG_DIAG_FIRST_FAIL (others: KG_ERR_INVALID_ARG).  Like
 * kg_row_eval it ignores kg_pod_row.elig_class (KG_WHY_ELIG is never set) and returns KG_ERR_UNSUPPORTED for a
 * cpuset pair on a node whose valid CPU topology lacks CPU detail. */
kg_status kg_row_why(const kg_config *cfg, const kg_node_row *node, const kg_pod_row *pod, int64_t now_ns,
                     uint32_t flags, uint32_t *why);

/* The reasons of up to KG_DIAG_MAX_PODS pods against every node of the shard (kg_set_shard) in one call: one
 * Diagnose per failed pod instead of one host call per node.  The pod rows travel with the call (as kg_cycle_one);
 * the batch uploaded with kg_pods_set is neither read nor replaced.  The snapshot is read as it is now (after
 * kg_place: the state after the batch's commits) and nothing is mutated: generation, rows and kg_counters.placed
 * stay; eval_calls + 1, evals + n * (E - B), out_bytes / h2d_bytes as for the other entries.
 *   counts  [n][KG_WHY_SLOTS] uint32 (required): counts[p][b], b = 0 and 1..27: the shard nodes whose word has bit b;
 *           slot KG_WHY_SLOT_REJECTED: nodes with a non-zero word other than ABSENT; slot KG_WHY_SLOT_FEASIBLE:
 *           nodes whose word is 0; the other slots 0.  Slots 0 + 30 + 31 sum to E - B.  Exact integers, identical
 *           from run to run (no atomics: per-(pod, tile) partial counts, then a sum over the tiles).
 *   pod_why [n] uint32 (may be NULL): the pod-level words
 *   why     [n][64 * W] uint32 (may be NULL): the words, kg_eval's plane contract - W = ceil((E - B) / 64), column c
 *           <=> node B + c, row stride 64 * W words, pad columns unspecified, nothing outside [n][64 * W] written,
 *           a device pointer 16-byte aligned, no pre-zeroing needed.
 * out_on_device != 0: the three pointers are device pointers on the engine's device.  The call returns after the
 * launches completed either way.  An empty shard writes all-zero counts only.
 * Errors (nothing launched): KG_ERR_RANGE for n > KG_DIAG_MAX_PODS, a row outside the engine bounds or an elig_class
 * outside the loaded classes; KG_ERR_INVALID_ARG for unknown flags, n < 0 or a null counts / pods with n > 0;
 * KG_ERR_STATE without a snapshot, on a stale engine, or for a quota index without a kg_quota_set group;
 * KG_ERR_UNSUPPORTED when Reservation is enabled with slots loaded (the restore changes NodeInfo per pair), under
 * NodeNUMAResource for a pod with KG_POD_NUMA_CPU_BIND or a snapshot holding a node with a CPU bind policy
 * (kg_cycle_one's rule), and for a pod with more than two NUMA hint lists. */
#define KG_WHY_SLOTS 32
#define KG_WHY_SLOT_REJECTED 30   /* nodes with a non-zero word other than ABSENT */
#define KG_WHY_SLOT_FEASIBLE 31   /* nodes whose word is 0 */
#define KG_DIAG_MAX_PODS 256
kg_status kg_diagnose(kg_engine *eng, const kg_pod_row *pods, int32_t n, int64_t now_ns, uint32_t flags,
                      uint32_t *counts, uint32_t *pod_why, uint32_t *why, int32_t out_on_device);

/* The k best feasible nodes of up to KG_CAND_MAX_PODS pods over every node of the shard (kg_set_shard) in one call,
 * with the score of each engine plugin: what a profile with Score plugins outside the engine needs instead of whole
 * planes (upstream numFeasibleNodesToFind + prioritizeNodes, but over 100 % of the nodes).  The pod rows travel with
 * the call (as kg_diagnose and kg_cycle_one); the batch uploaded with kg_pods_set is neither read nor replaced.  The
 * snapshot is read as it is now and nothing is mutated: generation, rows, quota state and kg_counters.placed /
 * resolved stay.  Node indices in the keys are global.
 *   keys       [n][k] uint64 (required): keys[p][j] is the (j + 1)-th best feasible node of pod p in
 *              kg_eval_out.top1's encoding, (total + 1) << 32 | (0xFFFFFFFF - node), total = sum of weight * score
 *              of the enabled engine plugins.  A list is strictly descending as uint64 (higher total first, among
 *              equal totals the lower node index first); entries at and past the pod's feasible count are 0.
 *   scores     [n][k][4] uint8 (may be NULL): {NodeResourcesFit, LoadAware, NodeNUMAResource, 0} scores (0..100) of
 *              the pair, 0 for a disabled plugin; all four bytes 0 where the key is 0.
 *   n_feasible [n] uint32 (may be NULL): the pod's feasible nodes in the shard.
 * Defining property: with the same rows on the same engine state loaded as a batch (kg_pods_set + kg_eval, no
 * reservation slots loaded), keys[p][0] == top1[p], the listed nodes are exactly the k largest keys formed from
 * mask / scores / numa_scores, and n_feasible[p] is the popcount of the pod's mask row - including everything
 * kg_eval folds into the mask: removed nodes, eligibility classes (elig_class) and the node-independent gates (a pod
 * that fails the ElasticQuota PreFilter against the device quota state, or requires a reservation with none loaded,
 * gets all-zero keys and n_feasible = 0).  Nodes outside the fp64 fast-path bounds are listed like any other (the
 * exact int64 pair path).  Totals stay within the tile-key width of the placement chunks (kg_config_validate's
 * weight limits).
 * Every cell of [n][k], [n][k][4] and [n] is written whatever the buffers held, nothing outside them, and a NULL
 * plane is not touched.  out_on_device != 0: the three pointers are device pointers on the engine's device (keys
 * 8-byte aligned, the others 4-byte aligned).  The call returns after the launches completed either way.  An empty
 * shard writes all-zero outputs and launches nothing; n = 0 is a no-op.
 * Exact integers, identical from run to run: per-(pod, tile) descending lists, then a k-way merge; no atomics, no
 * floating-point or order-dependent reduction.
 * Counters: eval_calls + 1, evals + n * (E - B), out_bytes by the bytes of the planes asked for, h2d_bytes by what
 * was uploaded.
 * Errors (nothing launched, nothing changed, counters untouched): KG_ERR_INVALID_ARG for flags != 0, n < 0 or a null
 * pods / keys with n > 0; KG_ERR_RANGE for k < 1, k > KG_CAND_MAX_K, n > KG_CAND_MAX_PODS, a row outside the engine
 * bounds or an elig_class outside the loaded classes; KG_ERR_STATE without a snapshot, on a stale engine, or for a
 * quota index without a kg_quota_set group; KG_ERR_UNSUPPORTED exactly where kg_diagnose refuses: Reservation
 * enabled with slots loaded, under NodeNUMAResource a pod with KG_POD_NUMA_CPU_BIND or a snapshot holding a node
 * with a CPU bind policy, and a pod with more than two NUMA hint lists.  KG_ERR_HIP when the engine-owned list
 * buffer ([n][tiles of the shard][k + 1] uint32) cannot be allocated; the engine stays usable. */
#define KG_CAND_MAX_K 64
#define KG_CAND_MAX_PODS 256
kg_status kg_candidates(kg_engine *eng, const kg_pod_row *pods, int32_t n, int64_t now_ns, int32_t k, uint32_t flags,
                        uint64_t *keys        /* [n][k], required */,
                        uint8_t  *scores      /* [n][k][4] = {fit, loadaware, numa, 0}; may be NULL */,
                        uint32_t *n_feasible  /* [n]; may be NULL */,
                        int32_t out_on_device);

/* The lists that several ranks or shards returned for the same n pods, combined on the host (no engine):
 * keys [n_lists][n][k], scores [n_lists][n][k][4] (may be NULL, then out_scores must be NULL too, and the reverse).
 * out_keys[p] is the k largest keys of the union, descending and zero-padded; out_scores follows its keys.
 * KG_ERR_INVALID_ARG, outputs untouched: n_lists < 1, n < 0, k outside 1..KG_CAND_MAX_K, null pointers, an input
 * list that is not strictly descending up to its first 0 or holds a non-zero key after a 0, or a non-zero key that
 * appears in two lists of one pod (the shards overlap). */
kg_status kg_candidates_merge(const uint64_t *keys, const uint8_t *scores /* may be NULL */, int32_t n_lists,
                              int32_t n, int32_t k, uint64_t *out_keys, uint8_t *out_scores /* NULL iff scores NULL */);

/* Preemption dry run: which pods would have to go, on which node, for a pod that fits nowhere (ElasticQuota's
 * PostFilter: elasticquota/plugin.go:302-321 runs the upstream preemption evaluator over every node,
 * preempt.go:43-45, with SelectVictimsOnNode of preempt.go:111-215).
 *
 * The bound-pod table is NodeInfo.Pods of every node of the snapshot (not of the shard): per node a list of at most
 * KG_BOUND_MAX_PER_NODE pods, each a kg_pod_row plus its priority (corev1helpers.PodPriority: Spec.Priority, 0 when
 * nil) and start time (Status.StartTime in ns; INT64_MAX for nil, where upstream takes Now(), later than every real
 * start).  Of a row the table keeps request / request_present / nonzero_request (the deltas of NodeInfo.RemovePod /
 * AddPodInfo), numa_request / numa_request_present (core.PodRequestsAndLimits, the quota deltas), quota and
 * flags & KG_POD_NON_PREEMPTIBLE; kg_bound_download returns exactly those, every other field of a row zero.
 * Position b of a pod in its node's list (the caller's order) is its identity in every output: bit b of a victim mask.
 * The engine keeps each list in util.MoreImportantPod order - higher priority first, then the earlier start; ties keep
 * the caller's order (the reference's sort.Slice leaves them unspecified) - and remembers each entry's position.
 * kg_bound_set replaces the whole table: first[n_nodes + 1] are CSR offsets into rows / priority / start_ns (first[0]
 * = 0, non-decreasing, no list longer than max_per_node), max_per_node (1..KG_BOUND_MAX_PER_NODE) the slots the table
 * keeps per node.  kg_bound_update replaces one node's list (n = 0 empties it).  kg_snapshot_reset drops the table;
 * kg_snapshot_upsert / _remove leave it alone.  The engine does not check that a node row's `requested` is the sum of
 * its list, and kg_place / kg_commit / kg_unreserve do not touch the table: the caller keeps it in step with
 * kg_bound_update the way it keeps rows in step with kg_snapshot_upsert.
 * Errors (nothing changed): KG_ERR_INVALID_ARG for null pointers; KG_ERR_STATE without a snapshot, and for
 * kg_bound_update / kg_bound_download before a kg_bound_set; KG_ERR_RANGE for a node or a count out of range (n or cap
 * above the table's max_per_node, a list longer than it), offsets that do not rise, or a row outside the engine bounds.
 * h2d_bytes grows by what was uploaded. */
#define KG_BOUND_MAX_PER_NODE 128
kg_status kg_bound_set(kg_engine *eng, const int32_t *first /* [n_nodes + 1], CSR offsets */, const kg_pod_row *rows,
                       const int32_t *priority, const int64_t *start_ns, int32_t max_per_node /* 1..128: the stride kept */);
kg_status kg_bound_update(kg_engine *eng, int32_t node, const kg_pod_row *rows, const int32_t *priority,
                          const int64_t *start_ns, int32_t n /* 0..max_per_node */);   /* replaces one node's list */
kg_status kg_bound_download(kg_engine *eng, int32_t node, kg_pod_row *rows, int32_t *priority, int64_t *start_ns,
                            int32_t cap, int32_t *n);   /* in the caller's order; for tests and debugging */

/* The dry run of one (preemptor, node) pair: preempt.go:111-215 restated, without PodDisruptionBudgets.
 *   1. a row that is not KG_NODE_VALID: KG_PRE_ABSENT.
 *   2. potential victims (canPreempt, preempt.go:283-294): not KG_POD_NON_PREEMPTIBLE, priority below the preemptor's,
 *      the same quota index (-1 equals -1).  None: KG_PRE_NO_VICTIMS ("No victims found", UnschedulableAndUnresolvable).
 *   3. all of them are removed from a copy of the row (requested -= request, nonzero_requested -= nonzero_request,
 *      pod_count - 1; LoadAware's la_used* stay: RemovePod does not reach the pod-assign cache; only Score reads
 *      NonZeroRequested, so the verdicts do not depend on it) and, when the quota
 *      check is active (ElasticQuota enabled and the preemptor's quota >= 0), from the group's `used`
 *      (quotav1.SubtractWithNonNegativeResult: max(0, used - numa_request) per resource, keys united; the ancestors
 *      and non_preemptible_used are neither read nor changed).
 *   4. Filter on the reduced row - exactly the verdict kg_row_why == 0 gives for it (kg_preempt adds the pod's
 *      eligibility class) - fails: KG_PRE_UNFIT.
 *   5. reprieve in importance order: the pod is added back to the row and to `used`; if the preemptor no longer fits
 *      it is removed again and becomes a victim; then, with the quota check active, used + numa_request must stay
 *      within used_limit on the resources both name (kg_quota_set's PreFilter compare on the evolving `used`): if not,
 *      a pod that still fits is removed and becomes a victim, and for a pod removed just above the reference removes
 *      it a second time, NodeInfo.RemovePod errors and the node is dropped: KG_PRE_ERROR (pinned, not repaired).
 *   6. KG_PRE_CANDIDATE with the victim mask (caller positions), n_victims, hi_prio (the highest victim priority),
 *      prio_sum (sum of priority + 2^31) and earliest_ns (the earliest start among the victims of priority hi_prio).  A
 *      candidate may have no victim: the pod fitted all along.
 * Every status but KG_PRE_CANDIDATE leaves the mask and the stats zero.
 * kg_row_preempt is the host entry (no engine; it ignores kg_pod_row.elig_class, as kg_row_why): bound[n_bound] in the
 * caller's order, quotas NULL <=> none.  KG_ERR_INVALID_ARG for null pointers, KG_ERR_RANGE for n_bound outside
 * 0..KG_BOUND_MAX_PER_NODE or an active quota index at or past n_quotas, KG_ERR_UNSUPPORTED with KG_PLUGIN_NUMA.
 * PodDisruptionBudgets are the PDB form below (kg_pdb_thresholds, kg_bound_pdb_set, kg_row_preempt_pdb); without
 * thresholds every potential victim is non-violating.
 * Out of scope (a caller that needs one of these keeps the host path): nominated pods
 * (RunFilterPluginsWithNominatedPods' add-back), PodEligibleToPreemptOthers (a host
 * check on one node), extenders, the eviction itself (the feeders deliver its pod deletes), NodeNUMAResource
 * (filterAmplifiedCPUs reads NodeInfo.Requested, so its verdict moves with every removal) and Reservation with slots
 * loaded (AddPod / RemovePod of its own, reservation/plugin.go:254-300). */
#define KG_PRE_CANDIDATE 0
#define KG_PRE_ABSENT 1
#define KG_PRE_NO_VICTIMS 2
#define KG_PRE_UNFIT 3
#define KG_PRE_ERROR 4
kg_status kg_row_preempt(const kg_config *cfg, const kg_node_row *node, const kg_pod_row *bound, const int32_t *bound_priority,
                         const int64_t *bound_start_ns, int32_t n_bound, const kg_pod_row *pod, int32_t pod_priority,
                         const kg_quota *quotas /* NULL <=> none */, int32_t n_quotas, int64_t now_ns,
                         int32_t *status, uint64_t victims[2], int64_t stats[4] /* n_victims, hi_prio, prio_sum, earliest_ns */);

/* The dry run of up to KG_PREEMPT_MAX_PODS preemptors against every node of the shard (kg_set_shard; node indices are
 * global) in one call, and the node to preempt on.  The pod rows travel with the call (as kg_diagnose); the batch
 * uploaded with kg_pods_set is neither read nor replaced.  Nothing is mutated: rows, table, quota state, generation and
 * kg_counters.placed / resolved stay.  The quota check reads group `used` / `used_limit` as the device holds them
 * (kg_quota_set and the commits since).
 *   pick  [n][KG_PREEMPT_PICK_WORDS] int64 (required): node (-1: no candidate), n_victims, hi_prio, prio_sum,
 *         earliest_ns, victim mask word 0, word 1, n_candidates (the KG_PRE_CANDIDATE nodes of the shard).  With node
 *         -1 every other word is 0.  The pick among the candidates restates upstream pickOneNodeForPreemption: a node
 *         with no victim wins outright, then the lowest hi_prio, the lowest prio_sum, the fewest victims, the latest
 *         earliest_ns, and last the lowest node index (upstream: map order; the project's tie rule).  With a PDB
 *         threshold plane loaded (below) word 1 also carries n_violating << 32, the second pick criterion.
 *   plane [n][64 * W] uint32 (may be NULL): status | n_victims << 8 | n_potential << 16 per node, kg_diagnose's plane
 *         contract - W = ceil((E - B) / 64), column c <=> node B + c, pad columns unspecified, nothing outside
 *         [n][64 * W] written, a device pointer 16-byte aligned, no pre-zeroing needed.
 * out_on_device != 0: both are device pointers on the engine's device (pick 8-byte aligned).  The call returns after
 * the launches completed either way.  Exact integers, identical from run to run: per-(pod, tile) best records, then a
 * reduction over the tiles; no atomics.  An empty shard writes node = -1 picks and launches nothing; n = 0 is a no-op.
 * kg_preempt_merge applies the same order on the host to the picks of several shards or ranks for the same pods
 * (picks [n_lists][n][8]); n_candidates is summed.  KG_ERR_INVALID_ARG for n_lists < 1, n < 0 or null pointers.
 * Counters: eval_calls + 1, evals + n * (E - B), out_bytes by the bytes of pick and plane, h2d_bytes by the upload.
 * Errors (nothing launched, counters untouched): KG_ERR_INVALID_ARG for flags != 0, n < 0 or a null pods / priority /
 * pick with n > 0; KG_ERR_RANGE for n > KG_PREEMPT_MAX_PODS, a row outside the engine bounds or an elig_class outside
 * the loaded classes; KG_ERR_STATE without a snapshot, without a bound table, on a stale engine, or for a quota index
 * without a kg_quota_set group; KG_ERR_UNSUPPORTED with KG_PLUGIN_NUMA enabled, or Reservation enabled with slots
 * loaded. */
#define KG_PREEMPT_MAX_PODS 64
#define KG_PREEMPT_PICK_WORDS 8
kg_status kg_preempt(kg_engine *eng, const kg_pod_row *pods, const int32_t *priority, int32_t n, int64_t now_ns, uint32_t flags /* 0 */,
                     int64_t *pick   /* [n][8], required */,
                     uint32_t *plane /* [n][64 * W], may be NULL */, int32_t out_on_device);
kg_status kg_preempt_merge(const int64_t *picks /* [n_lists][n][8] */, int32_t n_lists, int32_t n, int64_t *out /* [n][8] */);

/* PodDisruptionBudgets in the dry run (the PDB path of preempt.go:111-267).  filterPodsWithPDBViolation walks the
 * potential victims in importance order with one running budget per PDB; a victim at which a budget goes negative is
 * PDB-violating.  The violating ones are reprieved first, then the others, and numViolatingVictim is upstream's first
 * pick criterion after "a node with no victim".  The walk depends on the preemptor only through its priority and quota
 * group and folds into one threshold per bound pod: pod s is violating for a preemptor of priority P  <=>
 * pdb_prio(s) < P (INT32_MAX: never).  The PDB bookkeeping (namespaces, selectors, DisruptedPods) stays with the
 * caller, where the informers are.
 *
 * kg_pdb_thresholds (host, no engine) computes them for one node's list in the caller's order: pod b decrements the
 * PDBs pdb_ids[pdb_first[b] .. pdb_first[b + 1]) (indices into allowed[n_pdbs] = Status.DisruptionsAllowed; negative
 * counts as 0) - in the reference those of its namespace with a non-empty selector that matches its labels and
 * without its name in Status.DisruptedPods; a pod without labels has none.  Non-preemptible pods get INT32_MAX and
 * take part in no budget.  KG_ERR_INVALID_ARG for null pointers; KG_ERR_RANGE for n outside 0..KG_BOUND_MAX_PER_NODE,
 * offsets that do not start at 0 or do not rise, or an id outside [0, n_pdbs).
 * Recompute a node's thresholds after a bind, a delete or a priority change on it, and after a status change of a PDB
 * on every node that holds a pod the PDB covers.
 *
 * The engine keeps the thresholds in an optional plane beside the bound-pod table (allocated on first use; the table's
 * layout does not change).  kg_bound_pdb_set loads it for every node: `first` is kg_bound_set's CSR (every node's
 * length must equal the table's: KG_ERR_RANGE), pdb_prio in the caller's order; pdb_prio == NULL drops the plane.
 * kg_bound_pdb_update replaces one node's values (n must equal the node's count), kg_bound_pdb_download returns them
 * in the caller's order.  kg_bound_set and kg_snapshot_reset drop the plane; kg_bound_update resets that node's values
 * to INT32_MAX (the list changed: follow it with kg_bound_pdb_update).  Every rank of a sharded engine loads the same
 * plane.  KG_ERR_STATE without a table (and for _update / _download without a plane); KG_ERR_INVALID_ARG for null
 * pointers.  h2d_bytes grows by what was uploaded.
 *
 * With a plane loaded kg_preempt runs the PDB form: step 5 above runs twice over the list in importance order, first
 * over the violating potential victims, then over the others, and n_violating counts the pods of the first pass the
 * Fit verdict made victims (the reference increments on !fits alone: a first-pass pod that the quota re-check alone
 * makes a victim is a victim but is not counted; pinned, not repaired).  The mask, hi_prio, prio_sum and earliest_ns
 * do not depend on the order of the victims.  To rebuild the reference's victim list from the mask: the violating
 * victims (pdb_prio < P) in importance order, then the others in importance order.
 *   pick word 1 = n_victims | n_violating << 32; plane cell = status | n_victims << 8 | n_potential << 16 |
 *   n_violating << 24.  Both additions are zero without a plane.
 * The pick order becomes: a node with no victim, the fewest n_violating, then the order above; kg_preempt_merge
 * applies it too.  hi_prio stays the highest victim priority; the v1.24.15 evaluator reads victims.Pods[0], which with
 * victims of both kinds is the first violating one (a stated divergence; like the rest of the pick, parity unpinned).
 * kg_row_preempt_pdb is kg_row_preempt with bound_pdb_prio[n_bound] in the caller's order (NULL <=> none: the plain
 * form) and stats[4] = n_violating. */
kg_status kg_pdb_thresholds(const int32_t *priority, const int64_t *start_ns, const int32_t *quota,
                            const uint8_t *non_preemptible, int32_t n /* one node's list, caller order */,
                            const int32_t *pdb_first /* [n + 1] CSR */, const int32_t *pdb_ids,
                            const int32_t *allowed /* [n_pdbs] */, int32_t n_pdbs, int32_t *pdb_prio /* [n] out */);
kg_status kg_bound_pdb_set(kg_engine *eng, const int32_t *first /* [n_nodes + 1], as kg_bound_set */,
                           const int32_t *pdb_prio /* NULL: drop the plane */);
kg_status kg_bound_pdb_update(kg_engine *eng, int32_t node, const int32_t *pdb_prio, int32_t n);
kg_status kg_bound_pdb_download(kg_engine *eng, int32_t node, int32_t *out, int32_t cap, int32_t *n);
kg_status kg_row_preempt_pdb(const kg_config *cfg, const kg_node_row *node, const kg_pod_row *bound,
                             const int32_t *bound_priority, const int64_t *bound_start_ns,
                             const int32_t *bound_pdb_prio /* NULL <=> none */, int32_t n_bound, const kg_pod_row *pod,
                             int32_t pod_priority, const kg_quota *quotas /* NULL <=> none */, int32_t n_quotas,
                             int64_t now_ns, int32_t *status, uint64_t victims[2],
                             int64_t stats[5] /* n_victims, hi_prio, prio_sum, earliest_ns, n_violating */);

/* Measurement: when on, every k_eval launch (kg_eval, kg_place_chunk_eval) is bracketed by a
 * pair of HIP events on the engine stream (ring of 256).  kg_eval_kernel_times writes the
 * durations (ms) of the last min(n, recorded) launches, oldest first, and returns that count
 * (< 0 on error). */
kg_status kg_set_profiling(kg_engine *eng, int32_t on);
int32_t kg_eval_kernel_times(kg_engine *eng, float *ms, int32_t n);

/* Engine counters since creation or kg_counters_reset (SURVEY §5 "Metrics"; the reference's analogue is the
 * scheduler's Prometheus set, pkg/scheduler/metrics/metrics.go:28-41): pod×node pairs evaluated (matrix mode
 * and placement chunk evaluations), matrix-mode output bytes written, pods walked by placement resolves and
 * pods placed (kg_place / kg_commit, where the outcome reaches the host), host→device bytes uploaded, and the
 * device time of the k_eval launches timed under kg_set_profiling (evals ÷ that time = evals/s, output
 * bytes ÷ it = the achieved write rate). */
typedef struct kg_counters {
    uint64_t eval_calls;        /* kg_eval + kg_place_chunk_eval calls */
    uint64_t evals;             /* pod × node pairs evaluated */
    uint64_t out_bytes;         /* mask + score planes + top-1 bytes written by matrix mode */
    uint64_t resolved;          /* pods walked by placement resolves (kg_place, kg_place_chunk_resolve*) */
    uint64_t placed;            /* pods placed by kg_place / kg_commit */
    uint64_t h2d_bytes;         /* host → device bytes (snapshot rows, pod rows, class tables, reservations, ...) */
    uint64_t timed_launches;    /* k_eval launches whose device time is in kernel_ns */
    uint64_t kernel_ns;         /* their device time (HIP events, kg_set_profiling) */
} kg_counters;
kg_status kg_counters_get(kg_engine *eng, kg_counters *out);
kg_status kg_counters_reset(kg_engine *eng);

/* Helpers for consumers of matrix-mode output. */
static inline int kg_mask_test(const uint64_t *mask, int32_t n_nodes, int32_t p, int32_t n) {
    int32_t words = (n_nodes + 63) / 64;
    return (int)((mask[(int64_t)p * words + n / 64] >> (n % 64)) & 1u);
}

#ifdef __cplusplus
}
#endif
#endif /* KOORD_GPU_H */
