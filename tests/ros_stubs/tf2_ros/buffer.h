#pragma once
#include <geometry_msgs/TransformStamped.h>
namespace tf2_ros {
class Buffer {
 public:
  bool canTransform(const std::string &target_frame, const std::string &source_frame, const ros::Time &time, std::string *errstr) const;
  geometry_msgs::TransformStamped lookupTransform(const std::string &target_frame, const std::string &source_frame, const ros::Time &time) const;
};
}
