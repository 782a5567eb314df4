#pragma once
#include <geometry_msgs/Transform.h>
#include <std_msgs/ColorRGBA.h>
#include <std_msgs/Header.h>
namespace visualization_msgs {
struct Marker {   // visualization_msgs/Marker.msg
  enum { ARROW = 0, POINTS = 8 };
  enum { ADD = 0, MODIFY = 0, DELETE = 2, DELETEALL = 3 };
  std_msgs::Header header; std::string ns; int32_t id = 0, type = 0, action = 0;
  geometry_msgs::Pose pose; geometry_msgs::Vector3 scale; std_msgs::ColorRGBA color; ros::Duration lifetime; uint8_t frame_locked = 0;
  std::vector<geometry_msgs::Point> points; std::vector<std_msgs::ColorRGBA> colors;
  std::string text, mesh_resource; uint8_t mesh_use_embedded_materials = 0;
};
}
